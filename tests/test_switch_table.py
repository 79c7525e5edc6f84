"""The README's switch tables and the code name the same environment variables: every variable the library or the package reads
has a row, and every DD_ name in a row is read somewhere.  Host only; bench.py and tests/ are not scanned."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'deepdish_amd')
HEADING = '## A/B switches of the network engine'

C_READ = re.compile(r'\b(?:dd_env_int|dd_env_set|getenv)\(\s*"([A-Za-z0-9_]+)"')
PY_READ = re.compile(r'''os\.(?:environ\.get\(|environ\[|getenv\()\s*['"](DD_[A-Z0-9_]+)['"]''')
PY_IN = re.compile(r'''['"](DD_[A-Z0-9_]+)['"]\s+(?:not\s+)?in\s+os\.environ''')
NAME = re.compile(r'\bDD_[A-Z0-9_]*[A-Z0-9]\b')


def _read(path):
    with open(path, encoding='utf-8') as f:
        return f.read()


def names_read():
    got = {}
    for ext in ('hip', 'cpp', 'h'):
        for path in glob.glob(os.path.join(PKG, 'csrc', '*.' + ext)):
            for name in C_READ.findall(_read(path)):
                got.setdefault(name, os.path.relpath(path, ROOT))
    for path in glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True):
        text = _read(path)
        for name in PY_READ.findall(text) + PY_IN.findall(text):
            got.setdefault(name, os.path.relpath(path, ROOT))
    return got


def names_in_tables():
    """DD_ names in the table rows between the switch heading and the next heading."""
    lines = _read(os.path.join(ROOT, 'README.md')).splitlines()
    start = next(i for i, line in enumerate(lines) if line.startswith(HEADING))
    names = set()
    for line in lines[start + 1:]:
        if line.startswith('## '):
            break
        if line.startswith('|'):
            names.update(NAME.findall(line))
    return names


def test_scan_finds_both_languages():
    read = names_read()
    assert read['DD_WS'].endswith('nets.hip') and read['DD_Q_FUSE'].endswith('netsq.py') and read['DD_LIB'].endswith('_lib.py')


def test_every_variable_read_has_a_row():
    read, table = names_read(), names_in_tables()
    missing = {n: f for n, f in read.items() if n not in table}
    assert not missing, 'read in the code, no row in a README switch table: %s' % sorted(missing.items())


def test_every_row_names_a_variable_that_is_read():
    read, table = names_read(), names_in_tables()
    stale = sorted(table - set(read))
    assert not stale, 'named in a README switch table, read nowhere: %s' % stale
