"""motion_gate= of MultiStreamPipeline and HotPath, dd_pipeline_motion_gate: every refused form, by parameter name.  The Python refusals
are raised before anything is built and need no GPU; the C entry's own (DD_E_ARG / DD_E_STATE, the setter after the first step, the
other setters once the gate is set) need a pipeline and are marked gpu."""
import numpy as np
import pytest

S = 4
ON = dict(run_detector=False, background_subtraction_ratio=0.25, input_size=(64, 48))


def _refused(match, **kw):
    from deepdish_amd.multipipe import MultiStreamPipeline
    args = dict(ON)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        MultiStreamPipeline(S, context=object(), **args)        # (a context that cannot be used: nothing may get as far as needing it)


@pytest.mark.parametrize('bad', [-1, [0, 0, -3, 0], 1.5, [0.0, 1.0, 2.0, 3.0], 'zero', True, [0, 0, 0], [0] * 5, [[0, 0, 0, 0]], 2 ** 31,
                                 [None, 0, 0, 0]])
def test_a_threshold_of_the_wrong_sign_type_rank_or_length_is_refused(bad):
    _refused('motion_gate', motion_gate=bad)


def test_subtraction_off_is_refused():
    _refused('motion_gate.*background_subtraction_ratio', motion_gate=0, background_subtraction_ratio=None)
    _refused('motion_gate.*background_subtraction_ratio', motion_gate=[0] * S, background_subtraction_ratio=-1)


def test_a_ratio_of_zero_is_refused_because_an_empty_mask_then_decides_nothing():
    _refused('motion_gate.*background_subtraction_ratio = 0.*decides nothing', motion_gate=0, background_subtraction_ratio=0.0)
    _refused('motion_gate.*background_subtraction_ratio = 0', motion_gate=0, background_subtraction_ratio=[0.25, 0.25, 0.0, 0.5])


def test_either_form_of_skip_frames_with_some_n_above_zero_is_refused_as_not_built():
    _refused('motion_gate.*object_detector_skip_frames.*not built', motion_gate=0, object_detector_skip_frames=2)
    _refused('motion_gate.*object_detector_skip_frames.*not built', motion_gate=0, object_detector_skip_frames=[0, 0, 1, 0])
    _refused('motion_gate.*object_detector_skip_frames.*not built', motion_gate=0, object_detector_skip_frames=[1, 1, 1, 1],
             object_detector_skip_phase=[0, 1, 0, 1])


def test_hotpath_refuses_the_same_forms():
    from deepdish_amd.pipeline import HotPath
    on = dict(run_detector=False, disable_background_subtraction=False, input_size=(64, 48), context=object())
    for bad in (-1, 1.5, 'zero', True, [0]):
        with pytest.raises(ValueError, match='motion_gate'):
            HotPath(motion_gate=bad, **on)
    with pytest.raises(ValueError, match='motion_gate.*disable_background_subtraction'):
        HotPath(motion_gate=0, run_detector=False, context=object())
    with pytest.raises(ValueError, match='motion_gate.*background_subtraction_ratio'):
        HotPath(motion_gate=0, background_subtraction_ratio=0.0, **on)
    with pytest.raises(ValueError, match='motion_gate.*object_detector_skip_frames.*not built'):
        HotPath(motion_gate=0, object_detector_skip_frames=1, **on)


@pytest.mark.gpu
def test_the_c_entry_refuses_them_too_and_the_other_setters_keep_the_gate_consistent():
    import torch
    from deepdish_amd._lib import lib, DeepDishHipError
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import ptr
    DD_E_ARG, DD_E_STATE = -1, -3
    zero, neg, n1 = np.zeros(S, np.int32), np.array([0, 0, -1, 0], np.int32), np.array([0, 1, 0, 0], np.int32)
    off = MultiStreamPipeline(S, run_detector=False, input_size=(64, 48))
    assert lib().dd_pipeline_motion_gate(off._h, ptr(zero)) == DD_E_STATE and b'background subtraction is off' in lib().dd_last_error()
    mp = MultiStreamPipeline(S, **ON)
    assert lib().dd_pipeline_motion_gate(None, ptr(zero)) == DD_E_ARG
    assert lib().dd_pipeline_motion_gate(mp._h, None) == DD_E_ARG
    assert lib().dd_pipeline_motion_gate(mp._h, ptr(neg)) == DD_E_ARG and b'threshold[2] = -1' in lib().dd_last_error()
    r0 = MultiStreamPipeline(S, run_detector=False, input_size=(64, 48), background_subtraction_ratio=[0.25, 0.0, 0.25, 0.25])
    assert lib().dd_pipeline_motion_gate(r0._h, ptr(zero)) == DD_E_STATE and b'background_subtraction_ratio[1] = 0' in lib().dd_last_error()
    for skip in (2, [0, 0, 3, 0]):
        sk = MultiStreamPipeline(S, object_detector_skip_frames=skip, **ON)
        assert lib().dd_pipeline_motion_gate(sk._h, ptr(zero)) == DD_E_STATE
        assert b'object_detector_skip_frames' in lib().dd_last_error() and b'not built' in lib().dd_last_error()
    ok = MultiStreamPipeline(S, object_detector_skip_frames=[0] * S, **ON)      # per-stream counters with every N = 0 skip nothing
    assert lib().dd_pipeline_motion_gate(ok._h, ptr(zero)) == 0
    # an ungated pipeline reports nothing
    st = mp.gate_stats()
    assert st['steps'] == 0 and st['gated_stream_steps'] == 0 and st['count'].tolist() == [-1] * S and not st['gated'].any()
    # once set, the other setters refuse what the gate does not go with
    assert lib().dd_pipeline_motion_gate(mp._h, ptr(zero)) == 0
    assert lib().dd_pipeline_detector_skip_frames(mp._h, 2) == DD_E_STATE and b'motion gate' in lib().dd_last_error()
    assert lib().dd_pipeline_detector_skip_frames(mp._h, 0) == 0
    assert lib().dd_pipeline_detector_skip_streams(mp._h, ptr(n1), None) == DD_E_STATE and b'motion gate' in lib().dd_last_error()
    ratio0 = np.array([0.25, 0.25, 0.25, 0.0])
    assert lib().dd_pipeline_stream_motion_ratio(mp._h, ptr(ratio0)) == DD_E_STATE and b'motion' in lib().dd_last_error()
    for r in (None, 0.0):
        with pytest.raises(DeepDishHipError, match='motion gate'):
            mp.background_subtraction(r)
    # after the first step the gate can no longer be set or changed
    late = MultiStreamPipeline(S, **ON)
    for p in (mp, late):
        p.step(torch.zeros((S, p.H, p.W, 3), dtype=torch.uint8, device='cuda'))
        assert lib().dd_pipeline_motion_gate(p._h, ptr(zero)) == DD_E_STATE
        assert b'dd_pipeline_motion_gate' in lib().dd_last_error() and b'before the first step' in lib().dd_last_error()
    assert mp.gate_stats()['steps'] == 1 and late.gate_stats()['steps'] == 0
    assert late.motion_gate is None and MultiStreamPipeline(S, motion_gate=3, **ON).motion_gate.tolist() == [3] * S
    assert MultiStreamPipeline(S, motion_gate=np.array([0, 1, 2, 3]), **ON).motion_gate.tolist() == [0, 1, 2, 3]
