"""CPU: the op record has one statement on each side -- the OpWord enum of csrc/net_priv.h and nets.OP_FIELDS -- and the two agree, name for name
and index for index; so do the values of the hint word."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, 'deepdish_amd', 'csrc', 'net_priv.h')) as f:
        return f.read()


def test_word_enum_equals_the_python_table():
    from deepdish_amd import nets
    words = re.findall(r'^\s*W_(\w+) = (\d+),', _header(), re.M)
    assert len(words) >= 32 and len(set(n for n, _ in words)) == len(words)
    assert {n.lower(): int(i) for n, i in words} == nets.OP_FIELDS
    assert all(0 <= int(i) < nets.OP_WORDS for _, i in words)


def test_hint_values_and_record_size():
    from deepdish_amd import nets
    hints = {n: int(v) for n, v in re.findall(r'\b(HINT_\w+) = (\d+)', _header())}
    assert hints == {n: getattr(nets, n) for n in dir(nets) if n.startswith('HINT_')} and len(hints) == 5
    assert int(re.search(r'constexpr int OP_WORDS = (\d+);', _header()).group(1)) == nets.OP_WORDS
