"""GPU: chunk_rows_gather_k / chunk_rows_scatter_k alone (csrc/snapshot.hip, dd_chunk_rows_gather / dd_chunk_rows_scatter) against NumPy
indexing.  A gallery is a list of 32-row chunks scattered over arenas; gather packs the listed rows into a dense buffer in storage order,
scatter is the inverse.  Pure copies: every comparison is equality."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARENA_ROWS = 256                         # 8 chunks of 32 rows per arena
CPA = ARENA_ROWS // 32
ROWS = [0, 1, 31, 32, 33, 65]


def _call(fn, arenas, chunks, table, dense, dense_rows=None):
    from deepdish_amd._lib import lib
    from deepdish_amd.runtime import default_context, ptr
    ptrs = (ctypes.c_void_p * max(1, len(arenas)))(*[a.data_ptr() for a in arenas])
    chunks = np.ascontiguousarray(chunks, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    torch.cuda.synchronize()                 # torch fills its tensors on its own stream; the call below runs on the context's and waits for it itself
    return getattr(lib(), fn)(default_context().handle, ptrs, len(arenas), ARENA_ROWS, ptr(chunks) if chunks.size else None, int(chunks.size),
                              ptr(table) if table.size else None, len(table), ptr(dense), dense.shape[0] if dense_rows is None else dense_rows, None)


def _layout(rng, rows, n_arenas=2):
    """Chunk lists for entries of `rows` rows that alternate between the arenas, and a dense row for each with gaps between them."""
    free = [[a * CPA + c for c in rng.permutation(CPA)] for a in range(n_arenas)]
    chunks, table, at = [], [], 3
    for i, n in enumerate(rows):
        off = len(chunks)
        for k in range((n + 31) // 32):
            chunks.append(int(free[(i + k) % n_arenas].pop()))           # consecutive chunks of a list lie in different arenas
        table.append((off, n, at))
        at += n + 2
    return np.array(chunks, np.int32), np.array(table, np.int64).reshape(-1, 3), at + 3


def _expect_gather(arenas_np, chunks, table, dense0):
    out = dense0.copy()
    flat = np.concatenate(arenas_np)                                     # row of chunk c, row r: c * 32 + r (arenas of CPA chunks behind one another)
    for off, n, at in table:
        for r in range(n):
            out[at + r] = flat[chunks[off + r // 32] * 32 + r % 32]
    return out


def test_gather_and_scatter_equal_numpy_indexing():
    rng = np.random.default_rng(5)
    arenas_np = [rng.standard_normal((ARENA_ROWS, 128)).astype(np.float32) for _ in range(2)]
    arenas = [torch.from_numpy(a).cuda() for a in arenas_np]
    chunks, table, dense_rows = _layout(rng, ROWS)
    assert len({c // CPA for c in chunks[table[5][0]:table[5][0] + 3]}) == 2, 'a chunk list must jump between the arenas'
    dense0 = rng.standard_normal((dense_rows, 128)).astype(np.float32)
    dense = torch.from_numpy(dense0).cuda()
    assert _call('dd_chunk_rows_gather', arenas, chunks, table, dense) == 0
    got = dense.cpu().numpy()
    np.testing.assert_array_equal(got, _expect_gather(arenas_np, chunks, table, dense0))      # the rows around every destination untouched
    for a, b in zip(arenas, arenas_np):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    # scatter: the inverse, into OTHER chunks of fresh arenas -- then gathering those gives the dense rows back (the round trip)
    fresh_np = [rng.standard_normal((ARENA_ROWS, 128)).astype(np.float32) for _ in range(2)]
    fresh = [torch.from_numpy(a).cuda() for a in fresh_np]
    chunks2, table2, _ = _layout(np.random.default_rng(6), ROWS)
    table2[:, 2] = table[:, 2]
    assert not np.array_equal(chunks, chunks2)
    assert _call('dd_chunk_rows_scatter', fresh, chunks2, table2, dense) == 0
    want = np.concatenate(fresh_np)
    for off, n, at in table2:
        for r in range(n):
            want[chunks2[off + r // 32] * 32 + r % 32] = got[at + r]
    np.testing.assert_array_equal(np.concatenate([a.cpu().numpy() for a in fresh]), want)      # every other arena row untouched
    back = torch.zeros_like(dense)
    assert _call('dd_chunk_rows_gather', fresh, chunks2, table2, back) == 0
    for off, n, at in table:
        np.testing.assert_array_equal(back.cpu().numpy()[at:at + n], got[at:at + n])


def test_no_entries_and_refusals():
    from deepdish_amd._lib import lib
    arenas = [torch.zeros((ARENA_ROWS, 128), dtype=torch.float32, device='cuda') for _ in range(2)]
    dense = torch.full((40, 128), 7.0, dtype=torch.float32, device='cuda')
    assert _call('dd_chunk_rows_gather', arenas, [], np.zeros((0, 3)), dense) == 0            # an entry count of 0
    assert _call('dd_chunk_rows_scatter', arenas, [], np.zeros((0, 3)), dense) == 0
    assert _call('dd_chunk_rows_gather', arenas, [3], [(0, 0, 0)], dense) == 0                 # an entry of 0 rows
    assert float(dense.min()) == 7.0 and float(arenas[0].abs().max()) == 0.0
    for fn in ('dd_chunk_rows_gather', 'dd_chunk_rows_scatter'):
        assert _call(fn, arenas, [16], [(0, 1, 0)], dense) == -1 and b'chunks[0]' in lib().dd_last_error()          # chunk outside the arenas
        assert _call(fn, arenas, [1], [(0, 33, 0)], dense) == -1 and b'list of 1' in lib().dd_last_error()         # list too short for the rows
        assert _call(fn, arenas, [1, 2], [(0, 33, 8)], dense) == -1 and b'dense buffer of 40' in lib().dd_last_error()
        assert _call(fn, arenas, [1], [(0, -1, 0)], dense) == -1
    assert _call('dd_chunk_rows_gather', arenas, [1, 2], [(0, 4, 0), (1, 4, 3)], dense) == -1 and b'overlapping' in lib().dd_last_error()
    assert _call('dd_chunk_rows_scatter', arenas, [1, 1], [(0, 4, 0), (1, 4, 8)], dense) == -1 and b'written twice' in lib().dd_last_error()
    assert float(dense.min()) == 7.0 and float(arenas[0].abs().max()) == 0.0                      # a refused call launched nothing


def test_dense_rows_past_two_gib():
    """An entry whose dense destination starts at row 4 194 300 crosses byte 2^31 (row 4 194 304): one 2.2 GB buffer."""
    rng = np.random.default_rng(9)
    arenas_np = [rng.standard_normal((ARENA_ROWS, 128)).astype(np.float32) for _ in range(2)]
    arenas = [torch.from_numpy(a).cuda() for a in arenas_np]
    first, n = 4194300, 65
    dense_rows = first + n + 3
    dense = torch.zeros((dense_rows, 128), dtype=torch.float32, device='cuda')
    chunks = np.array([9, 2, 12], np.int32)
    table = [(0, n, first)]
    assert _call('dd_chunk_rows_gather', arenas, chunks, table, dense) == 0
    flat = np.concatenate(arenas_np)
    want = np.stack([flat[chunks[r // 32] * 32 + r % 32] for r in range(n)])
    tail = dense[first - 3:].cpu().numpy()
    np.testing.assert_array_equal(tail[3:3 + n], want)
    assert not tail[:3].any() and not tail[3 + n:].any()
    assert not bool(dense[:1024].any()), 'a 32-bit byte offset would have wrapped to the start of the buffer'
    # and back out of the far rows into other chunks
    fresh = [torch.zeros((ARENA_ROWS, 128), dtype=torch.float32, device='cuda') for _ in range(2)]
    chunks2 = np.array([0, 15, 7], np.int32)
    assert _call('dd_chunk_rows_scatter', fresh, chunks2, table, dense) == 0
    got = np.concatenate([a.cpu().numpy() for a in fresh])
    for r in range(n):
        np.testing.assert_array_equal(got[chunks2[r // 32] * 32 + r % 32], want[r])
    assert np.count_nonzero(got.any(axis=1)) == n
