"""CPU: the C-ABI library loads without a GPU and exports every symbol include/deepdish_hip.h declares;
the product never imports the oracle."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'deepdish_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(dd_[a-z0-9_]+)\s*\(', text)))


def test_every_declared_symbol_is_exported_and_bound():
    from deepdish_amd._lib import lib, MISSING, SIGNATURES, LIB_PATH
    l = lib()
    assert MISSING == []
    declared = _declared()
    assert len(declared) >= 35
    for name in declared:
        assert hasattr(l, name), 'declared in the header but not exported: ' + name
        assert name in SIGNATURES, 'declared in the header but not bound in _lib.py: ' + name
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dd_[a-z0-9_]+)', out))
    assert set(declared) <= exported
    assert l.dd_version() >= 100


def test_lanczos_plan_is_declared_and_answers_without_a_device():
    """dd_resize_lanczos_plan is in the header, the binary and the binding, and -- given the intermediate's address -- decides from the
    geometry and the alignments alone: no context, no GPU.  640x480 -> 300x300 is the one-launch form; 1080 rows are no multiple of 16, so
    a 1080p frame takes the scalar kernels (41 taps: not the LDS-row one); an odd row length takes the byte-wise vertical kernel."""
    import ctypes
    from deepdish_amd._lib import lib, SIGNATURES
    assert 'dd_resize_lanczos_plan' in _declared() and 'dd_resize_lanczos_plan' in SIGNATURES
    assert len(_declared()) >= 100

    def plan(H, W, c, swap, h, w, src=0x10000, dst=0x20040, tmp=0x30000):
        out = [ctypes.c_int(-1) for _ in range(4)]
        assert lib().dd_resize_lanczos_plan(None, H, W, c, swap, h, w, 1, src, dst, tmp, *[ctypes.byref(o) for o in out]) == 0
        return tuple(o.value for o in out)
    assert plan(480, 640, 3, 1, 300, 300) == (7, 6, 2, 1)          # DD_LANCZOS_H_FUSED, DD_LANCZOS_V_FUSED
    assert plan(720, 1280, 3, 1, 300, 300)[:2] == (5, 4)           # band wide, both passes
    assert plan(1080, 1920, 3, 1, 300, 300) == (4, 2, 0, 0)        # lanczos_h_k, lanczos_v4_k
    assert plan(1080, 1920, 3, 1, 640, 640) == (3, 2, 0, 0)        # lanczos_h_row_k
    assert plan(480, 640, 3, 1, 150, 150) == (4, 3, 0, 0)          # lanczos_v_k: 450-byte rows
    assert plan(480, 640, 3, 1, 300, 300, dst=0x20041) == (3, 3, 0, 0)      # a destination that is not 4-byte aligned: no dword stores
    assert plan(480, 640, 3, 0, 480, 640) == (0, 1, 0, 0) and plan(480, 640, 3, 0, 480, 640, dst=0x10000) == (0, 0, 0, 0)
    assert lib().dd_resize_lanczos_plan(None, 480, 640, 3, 1, 300, 300, 1, None, None, None, None, None, None, None) < 0      # neither a context nor tmp
    assert b'dd_resize_lanczos_plan' in lib().dd_last_error()
    assert lib().dd_resize_lanczos_plan(None, 480, 640, 2, 1, 300, 300, 1, None, None, 0x30000, None, None, None, None) < 0
    assert b'src_c' in lib().dd_last_error()


def test_errors_are_codes_not_exceptions():
    from deepdish_amd._lib import lib
    l = lib()
    assert l.dd_lsap_host(None, -1, 2, None, None) < 0
    assert b'dd_lsap_host' in l.dd_last_error()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'deepdish_amd')
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith('.py'):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), os.path.join(dp, fn)


def test_missing_library_is_a_loud_error(tmp_path):
    code = ("import deepdish_amd._lib as l; l.LIB_PATH = %r; l._lib = None\n"
            "try:\n    l.lib()\nexcept l.DeepDishHipError as e:\n    print('LOUD', e)\n" % str(tmp_path / 'nope.so'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT).stdout
    assert 'LOUD' in out and 'no CPU fallback' in out
