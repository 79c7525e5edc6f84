"""CPU: the helpers of deepdish_amd/multipipe.py that take a per-stream parameter apart before anything is built -- every accepted form
gives its result, every refused one is a ValueError that names the parameter."""
import numpy as np
import pytest

from deepdish_amd.multipipe import _stream_values, _stream_lines, _stream_wanted, _stream_ratio, _reset_streams

W, H = 640, 480


# ------------------------------------------------------------------ numbers
@pytest.mark.parametrize('what,integer', [('max_age', True), ('n_init', True), ('max_cosine_distance', False), ('max_iou_distance', False),
                                          ('nms_max_overlap', False)])
def test_stream_values_forms(what, integer):
    dt = np.int32 if integer else np.float64
    for S in (1, 4):
        a = _stream_values(3, what, S, integer)                          # a Python scalar
        assert a.dtype == dt and a.tolist() == [3] * S and a.flags.c_contiguous
        assert _stream_values(np.float64(3), what, S, integer).tolist() == [3] * S          # a NumPy scalar (int(60.0), as always)
        seq = list(range(1, S + 1))
        b = _stream_values(seq, what, S, integer)                        # a sequence of exactly S
        assert b.dtype == dt and b.tolist() == seq
        assert _stream_values(np.array(seq), what, S, integer).tolist() == seq
        assert _stream_values(tuple(seq), what, S, integer).tolist() == seq
    if not integer:
        assert _stream_values([0.2, 0.5], what, 2).tolist() == [0.2, 0.5]
        assert _stream_values(0.25, what, 3).tolist() == [0.25] * 3


@pytest.mark.parametrize('what,integer', [('max_age', True), ('n_init', True), ('max_cosine_distance', False), ('max_iou_distance', False),
                                          ('nms_max_overlap', False)])
def test_stream_values_refusals_name_the_parameter(what, integer):
    bad = [[1, 2, 3], [1, 2, 3, 4, 5], [[1, 2, 3, 4]], np.ones((4, 1)), 'x', ['a', 'b', 'c', 'd'], None, [1, 2, -1, 4]]
    bad += [[1.5, 2, 3, 4], [1, 2, float('nan'), 4]] if integer else [[1, 2, float('nan'), 4], [1, float('inf'), 3, 4], float('nan')]
    for v in bad:
        with pytest.raises(ValueError, match=what):
            _stream_values(v, what, 4, integer)
    with pytest.raises(ValueError, match=what):
        _stream_values([1, 2], what, 1, integer)                         # S == 1 takes one value, not two


# ------------------------------------------------------------------ lines
def test_stream_lines_forms():
    default = [W / 2, 0, W / 2, H]                                       # deepdish.py:739-741
    for S in (1, 4):
        a = _stream_lines(None, S, W, H)
        assert a.shape == (S, 4) and a.dtype == np.float64 and a.flags.c_contiguous and a.tolist() == [default] * S
        for one in ([10, 20, 30, 40], [[10, 20], [30, 40]], np.array([10., 20., 30., 40.]), (10, 20, 30, 40)):
            assert _stream_lines(one, S, W, H).tolist() == [[10, 20, 30, 40]] * S
    per = np.arange(16, dtype=float).reshape(4, 4)
    np.testing.assert_array_equal(_stream_lines(per, 4, W, H), per)
    np.testing.assert_array_equal(_stream_lines(per.reshape(4, 2, 2), 4, W, H), per)
    np.testing.assert_array_equal(_stream_lines(per.tolist(), 4, W, H), per)
    np.testing.assert_array_equal(_stream_lines(per[:1], 1, W, H), per[:1])            # S == 1: (1, 4) and (1, 2, 2)
    np.testing.assert_array_equal(_stream_lines(per[:1].reshape(1, 2, 2), 1, W, H), per[:1])
    # a size == 4 value stays the pipeline's line whatever S is
    np.testing.assert_array_equal(_stream_lines([[1, 2], [3, 4]], 2, W, H), [[1, 2, 3, 4]] * 2)


def test_stream_lines_refusals():
    per = np.arange(16, dtype=float).reshape(4, 4)
    nan, inf = per.copy(), per.copy()
    nan[2, 1], inf[0, 3] = np.nan, -np.inf
    for bad in (per[:3], per.reshape(2, 8), per.reshape(4, 4, 1), per.reshape(2, 2, 2, 2), [1, 2, 3], [1, 2, 3, 4, 5], nan, inf,
                [1, 2, 3, float('nan')], 'x1,y1,x2,y2', [[1, 2, 3, 4], [1, 2, 3]]):
        with pytest.raises(ValueError, match='line'):
            _stream_lines(bad, 4, W, H)
    with pytest.raises(ValueError, match='line'):
        _stream_lines(per, 1, W, H)


# ------------------------------------------------------------------ wanted labels
def test_stream_wanted_forms_and_union_order():
    for S in (1, 4):
        assert _stream_wanted(('person',), S) == (['person'], None)
        assert _stream_wanted(['car', 'bus', 'truck', 'bicycle'], S) == (['car', 'bus', 'truck', 'bicycle'], None)
        assert _stream_wanted([], S) == ([], None)
    assert _stream_wanted([['person']], 1) == (['person'], [['person']])
    assert _stream_wanted([[]], 1) == ([], [[]])
    # the union: order of first appearance, scanning streams 0 .. S - 1; every stream keeps its own order
    per = [['car', 'bus'], ['person'], ['bus', 'person', 'truck', 'car'], []]
    union, own = _stream_wanted(per, 4)
    assert union == ['car', 'bus', 'person', 'truck'] and own == per
    union, own = _stream_wanted((('b', 'a'), ('a', 'b')), 2)
    assert union == ['b', 'a'] and own == [['b', 'a'], ['a', 'b']]
    assert _stream_wanted([['a'], ['a']], 2) == (['a'], [['a'], ['a']])


def test_stream_wanted_refusals():
    for bad, S in (('person', 1), ('person', 6), (b'person', 1), (None, 2), ([['a'], ['b']], 3), ([['a'], ['b'], ['c']], 2), ([['a'], 'b'], 2),
                   (['a', ['b']], 2), ([['a'], [1]], 2), ([['a'], 3], 2), ([[['a']], ['b']], 2), ([['a']], 4)):
        with pytest.raises(ValueError, match='wanted_labels'):
            _stream_wanted(bad, S)


# ------------------------------------------------------------------ background subtraction ratio
def test_stream_ratio_forms():
    for S in (1, 3):
        assert _stream_ratio(None, S) is None
        assert _stream_ratio(-1, S) is None and _stream_ratio(-0.5, S) is None          # one negative value = off, as always
        assert _stream_ratio(0.25, S).tolist() == [0.25] * S and _stream_ratio(np.float32(0.5), S).tolist() == [0.5] * S
        assert _stream_ratio(0, S).tolist() == [0.0] * S
    a = _stream_ratio([0.0, 0.25, 1.0], 3)
    assert a.dtype == np.float64 and a.tolist() == [0.0, 0.25, 1.0]
    assert _stream_ratio(np.array([0.9]), 1).tolist() == [0.9]


def test_stream_ratio_refusals():
    for bad, S in (([0.25, None, 0.25], 3), ([0.25, -1, 0.25], 3), ([0.25, 1.5, 0.25], 3), ([0.25, float('nan'), 0.25], 3), ([0.25, 0.25], 3),
                   ([0.25] * 4, 3), ([[0.25, 0.25, 0.25]], 3), ('0.25', 3), (['a', 'b', 'c'], 3), ([0.1, 0.2], 1)):
        with pytest.raises(ValueError, match='background_subtraction_ratio'):
            _stream_ratio(bad, S)


# ------------------------------------------------------------------ reset
def test_reset_streams_list():
    assert _reset_streams([], 3).tolist() == [] and _reset_streams((), 1).size == 0
    a = _reset_streams([2, 0], 3)
    assert a.dtype == np.int32 and a.tolist() == [2, 0]
    assert _reset_streams(np.array([0]), 1).tolist() == [0]
    for bad in ([3], [-1], [0, 0], [1, 2, 1], [0.5], [[0, 1]]):
        with pytest.raises(ValueError, match='streams'):
            _reset_streams(bad, 3)
