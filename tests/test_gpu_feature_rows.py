"""GPU: dd_feature_rows_carry (csrc/featrows.hip, feature_rows_carry_k) against numpy indexing -- equality.  No streams, a stream with no
rows, one row, three streams with (5, 0, 7) rows from both sources, 300 streams, the bytes around both destinations untouched, a source
row past 2^31 bytes, and the ranges the host refuses."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW = 128
GUARD = 3                                # rows of sentinel before and after each destination
SENTINEL = -7.5


def _carry(fresh, store, out, store_out, table, out_off=0, store_off=0):
    """Tensors are f32 [rows, 128] (or None); out / store_out are handed over from row out_off / store_off on."""
    from deepdish_amd._lib import lib
    from deepdish_amd.runtime import default_context
    tb = np.ascontiguousarray(np.asarray(table, dtype=np.int32).reshape(-1, 6))
    P = ctypes.c_void_p

    def at(t, row=0):
        return P(None) if t is None else P(t.data_ptr() + row * ROW * 4)

    def rows(t, row=0):
        return 0 if t is None else t.shape[0] - row
    # (a destination handed over from row k on has k guard rows at its end as well: they are not part of it)
    return lib().dd_feature_rows_carry(default_context().handle, at(fresh), rows(fresh), at(store), rows(store), at(out, out_off),
                                       rows(out, 2 * out_off), at(store_out, store_off), rows(store_out, 2 * store_off),
                                       tb.ctypes.data_as(P), len(tb), None)


def _run_and_check(table, n_fresh, n_store, seed):
    """Runs the table over random sources; both destinations are sized to what the table writes, with guard rows around them."""
    rng = np.random.default_rng(seed)
    tb = np.asarray(table, dtype=np.int64).reshape(-1, 6)
    fresh = rng.standard_normal((max(n_fresh, 1), ROW)).astype(np.float32)
    store = rng.standard_normal((max(n_store, 1), ROW)).astype(np.float32)
    n_out = int((tb[:, 3] + tb[:, 2])[tb[:, 2] > 0].max()) if (tb[:, 2] > 0).any() else 0
    n_new = int((tb[:, 5] + tb[:, 4])[tb[:, 4] > 0].max()) if (tb[:, 4] > 0).any() else 0
    out = torch.full((n_out + 2 * GUARD, ROW), SENTINEL, dtype=torch.float32, device='cuda')
    new = torch.full((n_new + 2 * GUARD, ROW), SENTINEL, dtype=torch.float32, device='cuda')
    assert _carry(torch.from_numpy(fresh).cuda(), torch.from_numpy(store).cuda(), out, new, tb, GUARD, GUARD) == 0
    want_out = np.full((n_out + 2 * GUARD, ROW), SENTINEL, np.float32)
    want_new = np.full((n_new + 2 * GUARD, ROW), SENTINEL, np.float32)
    for sel, src, no, do, ns, dst in tb:
        rows = (store if sel else fresh)
        want_out[GUARD + do:GUARD + do + no] = rows[src:src + no]
        want_new[GUARD + dst:GUARD + dst + ns] = rows[src:src + ns]
    np.testing.assert_array_equal(out.cpu().numpy(), want_out)
    np.testing.assert_array_equal(new.cpu().numpy(), want_new)


def test_no_streams_and_a_stream_without_rows_launch_nothing():
    assert _carry(None, None, None, None, np.zeros((0, 6))) == 0
    _run_and_check([[0, 0, 0, 0, 0, 0]], 4, 4, 1)
    _run_and_check([[1, 2, 0, 0, 0, 0]], 4, 4, 2)


@pytest.mark.parametrize('sel', [0, 1])
def test_one_row(sel):
    _run_and_check([[sel, 2, 1, 0, 1, 0]], 4, 4, 3 + sel)
    _run_and_check([[sel, 3, 1, 0, 0, 0]], 4, 4, 5 + sel)      # to the tracker's input only
    _run_and_check([[sel, 0, 0, 0, 1, 0]], 4, 4, 7 + sel)      # to the store only


def test_three_streams_from_mixed_sources():
    """(5, 0, 7) rows: stream 0 fresh -> tracker input and store; stream 1 nothing; stream 2 from the store, 4 of its 7 retained rows go to
    the tracker (zip truncation) while all 7 are carried; then the same with the destinations in another order."""
    _run_and_check([[0, 3, 5, 0, 5, 0], [1, 0, 0, 5, 0, 5], [1, 2, 4, 5, 7, 5]], 9, 10, 11)
    _run_and_check([[1, 1, 5, 7, 5, 7], [0, 0, 0, 0, 0, 0], [0, 0, 7, 0, 3, 1]], 9, 10, 12)


def test_three_hundred_streams():
    """Rows 0 .. 12 per stream, sources alternating, a third of the streams absent from the tracker's input, every ninth not carried."""
    rng = np.random.default_rng(21)
    S = 300
    cnt = rng.integers(0, 13, S)
    tb, fr, so, o, d = [], 0, 0, 0, 0
    for z in range(S):
        sel, n = z % 2, int(cnt[z])
        n_out = 0 if z % 3 == 2 else int(rng.integers(0, n + 1))
        n_store = 0 if z % 9 == 4 else n
        tb.append([sel, so if sel else fr, n_out, o, n_store, d])
        fr, so = fr + (0 if sel else n), so + (n if sel else 0)
        o, d = o + n_out, d + n_store
    _run_and_check(tb, fr, so, 22)


def test_a_source_row_past_2_to_the_31_bytes():
    """Row 4 194 310 of the fresh buffer starts past 2^31 bytes: the allocation is left uninitialised, only the rows read are written."""
    first, n = 4194304 + 6, 3
    assert first * ROW * 4 > 2 ** 31
    fresh = torch.empty((first + n, ROW), dtype=torch.float32, device='cuda')
    rows = torch.from_numpy(np.random.default_rng(31).standard_normal((n, ROW)).astype(np.float32)).cuda()
    fresh[first:] = rows
    out = torch.full((n + 2 * GUARD, ROW), SENTINEL, dtype=torch.float32, device='cuda')
    new = torch.full((n + 2 * GUARD, ROW), SENTINEL, dtype=torch.float32, device='cuda')
    assert _carry(fresh, None, out, new, [[0, first, n, 0, n - 1, 0]], GUARD, GUARD) == 0
    want = np.full((n + 2 * GUARD, ROW), SENTINEL, np.float32)
    want[GUARD:GUARD + n] = rows.cpu().numpy()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    want[GUARD + n - 1] = SENTINEL
    np.testing.assert_array_equal(new.cpu().numpy(), want)


def test_bad_ranges_are_refused_on_the_host():
    from deepdish_amd._lib import lib
    src = torch.zeros((4, ROW), dtype=torch.float32, device='cuda')
    out = torch.full((4, ROW), SENTINEL, dtype=torch.float32, device='cuda')
    new = torch.full((4, ROW), SENTINEL, dtype=torch.float32, device='cuda')
    for table in ([[0, 3, 2, 0, 0, 0]],              # reads past the fresh rows
                  [[1, -1, 1, 0, 0, 0]],             # a negative source row
                  [[0, 0, 2, 3, 0, 0]],              # writes past the output
                  [[0, 0, 0, 0, 2, 3]],              # writes past the next store
                  [[2, 0, 1, 0, 0, 0]],              # no such source
                  [[0, 0, -1, 0, 0, 0]],
                  [[0, 0, 2, 0, 0, 0], [1, 0, 2, 1, 0, 0]]):      # two streams write row 1 of the output
        assert _carry(src, src, out, new, table) == -1, table
        assert b'dd_feature_rows_carry' in lib().dd_last_error()
    assert _carry(None, src, out, new, [[0, 0, 1, 0, 0, 0]]) == -1      # rows asked of a source that is not there
    assert (out.cpu().numpy() == SENTINEL).all() and (new.cpu().numpy() == SENTINEL).all()
