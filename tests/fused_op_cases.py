"""The cases of tests/test_gpu_fused_ops.py and tests/test_fused_op_ref.py: the smallest program that reaches each fused launch of the f16 engine,
the launch codes its ops must report and the float64 reference of what the launch computes.

A case is a program on a `Rig` (tests/net_op_rig.py): a u8 input, 1x1 feeders whose tensors are read back (the reference's inputs), then the
op(s) under test with the hint words compile_mars / compile_ssd_mobilenet set.  `codes` is what dd_net_op_launches must report for those ops, in
program order -- literals, written down from reading run_conv, run_conv3x3_rw, run_stem, run_dwpw, run_dwconv and the *_eligible / *_fusable /
mars_pair_match functions of csrc/nets.hip once, not recomputed from a copy of their rules.  `chunk` is a crop count below every threshold of the
ops involved: in chunks of that size the same engine runs the same ops on the layer-by-layer kernels, whose tensors the fused launch's must equal
bit for bit (mars_ws128_k runs at every crop count: no chunk).

Crop counts.  CU = 256 on the MI355X, and several launchers carry that literal: the GPU tests assert it.  mars_ws128_k and mars_pair64_k give
crop n to workgroup n % min(n, CU); the deepest ring of mars_ws128_k is WS_NBR = 5 residual slots (4 tile slots), of mars_pair64_k 3 residual
tiles: 5 CU + 1 and 3 CU + 1 crops give workgroup 0 one more crop than that ring has slots.  The row kernels give a wave (or a wave pair) a crop
and stream its rows through row rings; their counts are the dispatch threshold, one more (an odd tail) and a count past one full round of the
grid (2049 = 4 waves x 512 workgroups + 1).
"""
import numpy as np

import net_op_ref as R
import net_op_cases as C
from net_op_ref import ACT_NONE, ACT_RELU6, ACT_ELU

CU = 256
OPK_DEFAULT, OPK_FOLDED, OPK_FOLDED_PREV = 0, 1, 15
OPK_POOL_ROWS, OPK_POOL_ROWS_STEM, OPK_RES_UNIT, OPK_SSD_FRONT, OPK_C64_ROWS, OPK_S2_ROWS, OPK_CONV_WS, OPK_WS_DW = 2, 3, 4, 5, 6, 7, 8, 9
OPK_DWPW_ROWS, OPK_RES_PAIR, OPK_MARS_WS, OPK_MARS_PAIR, OPK_STEM_WIDE = 10, 12, 14, 16, 23
FUSED_CODES = {2, 3, 4, 5, 6, 7, 9, 10, 12, 14, 16, 23}
HINT_NEXT_ONLY, HINT_HOLD_UNIT, HINT_NEXT_IS_PROJ, HINT_PAIR_MEMBER = 1, 2, 3, 4        # deepdish_amd/nets.py


def L(hw, k, cin, cout, stride=1, pad=1, act=ACT_NONE, res=False, dst2=False, pool=False, splitk=1):
    """One dense layer of a case (geometry and seeded weights of net_op_cases.Conv; the variant word is not used here)."""
    return C.Conv('', hw, 3, k, cin, cout, (0, 0, 0, 0, 0, 0, splitk), stride=stride, pad=pad, act=act, res=res, dst2=dst2, pool=pool)


def _a(layer):
    return (R.f16(layer.w), layer.b, layer.stride, layer.pad_t, layer.pad_l, layer.ho, layer.wo)


class Fused:
    """kind: how the program is built and which reference it is held to (build / reference below).  counts: crops per forward.  codes: launch
    codes of the ops under test.  chunk: crops per forward of the layer-by-layer run (None: the launch has no other path, or is that path).  wg:
    crop -> workgroup that computes (the first row of) it, given the crop count.  env: switches read on every forward.  ref_crops: the crops the
    float64 reference is computed for where every crop would take minutes (with workgroup 0's; negative = from the end)."""

    def __init__(self, name, kind, hw, layers, counts, codes, chunk, wg, seeds=None, env=None, ref_crops=None):
        self.name, self.kind, (self.H, self.W), self.layers, self.counts, self.codes, self.chunk, self.wg = name, kind, hw, layers, counts, codes, chunk, wg
        self.env, self.ref_crops = env or {}, ref_crops
        self.program_input = kind not in ('stempool', 'ssdfront', 'stemwide')          # those read the u8 crops themselves
        for i, l in enumerate(layers):
            if isinstance(l, C.Conv):
                l.w, l.b, l.aff2 = C.conv_weights(l, seed=(seeds or range(31, 31 + len(layers)))[i])

    def __repr__(self):
        return self.name


def wg_crop(n):             # mars_ws128_k, mars_pair64_k: one workgroup per CU, crops n0, n0 + grid, ...
    return np.arange(n) % min(n, CU)


def wg_wave4(n):            # res_unit_rows_k, conv3x3_s2_rows_k: a wave per crop, four waves a workgroup, two workgroups per CU
    return (np.arange(n) // 4) % min(-(-n // 4), 2 * CU)


def wg_pair4(n):            # res_pair_rows_k: a wave pair per crop, four pairs a workgroup, one workgroup per CU
    return (np.arange(n) // 4) % min(-(-n // 4), CU)


def wg_wave2(n):            # conv3x3_c64_rows_k: two crops a workgroup (two channel halves each)
    return (np.arange(n) // 2) % min(-(-n // 2), 2 * CU)


def wg_pool_rows(n):        # conv3x3_pool_rows_k: a crop is 4 / 2 / 1 units (below 768 / below 1536 crops / from there), four units a workgroup
    split = 1 if n >= 1536 else 2 if n >= 768 else 4
    return (np.arange(n) * split // 4) % min(-(-n * split // 4), 2 * CU)


def wg_tasks(per_crop):
    """ssd_front_k / dwpw_rows_k: a crop is strips x parts tasks (launch_ssd_front, launch_dwpw_rows), four tasks a workgroup; per_crop(n) = that
    product at n crops."""
    def f(n):
        t = per_crop(n)
        return (np.arange(n) * t // 4) % min(-(-n * t // 4), 2 * CU)
    return f


def wg_stem_wide(width):
    """stem_conv_pool_wide_k: 4 / (width / 32) crops a workgroup, each group of crops 4 / 2 / 1 units (below 256 / below 512 groups / from there)."""
    def f(n):
        cpw = 4 // (width // 32)
        groups = -(-n // cpw)
        split = 1 if groups >= 512 else 2 if groups >= 256 else 4
        return (np.arange(n) // cpw * split) % min(groups * split, 2 * CU)
    return f


def wg_ws_dw(n_workers):
    """conv_ws_dw_k: 512 workgroups = n_workers workers x channel slices; worker w owns frames [w n / n_workers, (w + 1) n / n_workers)."""
    return lambda n: np.minimum(((np.arange(n) + 1) * n_workers - 1) // n, n_workers - 1)


def _parts(n, strips, rows, extra):
    """The row parts per strip launch_ssd_front (extra 2) / launch_dwpw_rows (extra 3) choose."""
    best, parts = None, 1
    for p in range(1, 9):
        cost = ((n * strips * p + 2047) // 2048) * (-(-rows // p) + extra)
        if best is None or cost < best:
            best, parts = cost, p
    return parts


WS_COUNTS = (1, 2, 3, CU - 1, CU, CU + 1, 2 * CU + 1, 5 * CU + 1)
PAIR64_COUNTS = (256, 257, 2 * CU + 1, 3 * CU + 1)
ROW_COUNTS = (512, 513, 2049)

CASES = [
    # ---- mars_ws128_k (csrc/mars_tail.hip): every crop count, no other path in the process
    Fused('ws128_s1_elu', 'conv', (8, 4), [L((8, 4), 3, 128, 128, act=ACT_ELU, splitk=2)], WS_COUNTS, (OPK_MARS_WS,), None, wg_crop),
    Fused('ws128_s1_res', 'conv', (8, 4), [L((8, 4), 3, 128, 128, res=True, splitk=2)], WS_COUNTS, (OPK_MARS_WS,), None, wg_crop),
    Fused('ws128_s1_res_out2', 'conv', (8, 4), [L((8, 4), 3, 128, 128, res=True, dst2=True, splitk=2)], WS_COUNTS, (OPK_MARS_WS,), None, wg_crop),
    Fused('ws128_s2_proj', 's2proj', (16, 8), [L((16, 8), 3, 64, 128, stride=2, pad=None, act=ACT_ELU, splitk=2),
                                              L((16, 8), 1, 64, 128, stride=2, pad=0, splitk=2)], WS_COUNTS, (OPK_MARS_WS, OPK_FOLDED_PREV), None, wg_crop),
    # ---- mars_pair64_k (csrc/mars_pair.hip), from 256 crops
    Fused('pair64_first', 'projblock', (31, 15), [L((31, 15), 3, 32, 64, stride=2, act=ACT_ELU), L((31, 15), 1, 32, 64, stride=2, pad=0),
                                                 L((16, 8), 3, 64, 64, res=True, dst2=True)], PAIR64_COUNTS, (OPK_FOLDED, OPK_FOLDED, OPK_MARS_PAIR), 255, wg_crop),
    Fused('pair64_second', 'unit', (16, 8), [L((16, 8), 3, 64, 64, act=ACT_ELU), L((16, 8), 3, 64, 64, res=True, dst2=True)], PAIR64_COUNTS,
          (OPK_FOLDED, OPK_MARS_PAIR), 255, wg_crop),
    # ---- the row pipelines of conv2_x / conv3_x, from 512 (1024) crops
    Fused('res_unit', 'unit_self', (31, 15), [L((31, 15), 3, 32, 32, act=ACT_ELU), L((31, 15), 3, 32, 32, res=True, dst2=True)], ROW_COUNTS,
          (OPK_FOLDED, OPK_RES_UNIT), 511, wg_wave4),
    Fused('res_unit_raw_sep', 'unit', (31, 15), [L((31, 15), 3, 32, 32, act=ACT_ELU), L((31, 15), 3, 32, 32, res=True, dst2=True)], ROW_COUNTS,
          (OPK_FOLDED, OPK_RES_UNIT), 511, wg_wave4),
    Fused('res_pair', 'pair', (31, 15), [L((31, 15), 3, 32, 32, act=ACT_ELU), L((31, 15), 3, 32, 32, res=True, dst2=True),
                                        L((31, 15), 3, 32, 32, act=ACT_ELU), L((31, 15), 3, 32, 32, res=True, dst2=True)], (1024, 1025, 2049),
          (OPK_FOLDED, OPK_FOLDED, OPK_FOLDED, OPK_RES_PAIR), 511, wg_pair4),
    Fused('s2_rows', 'conv', (31, 15), [L((31, 15), 3, 32, 64, stride=2, act=ACT_ELU)], ROW_COUNTS, (OPK_S2_ROWS,), 511, wg_wave4),
    Fused('c64_rows_elu', 'conv', (16, 8), [L((16, 8), 3, 64, 64, act=ACT_ELU)], ROW_COUNTS, (OPK_C64_ROWS,), 511, wg_wave2),
    Fused('c64_rows_res_out2', 'conv', (16, 8), [L((16, 8), 3, 64, 64, res=True, dst2=True)], ROW_COUNTS, (OPK_C64_ROWS,), 511, wg_wave2),
    # ---- the front of the 64 x 32 encoder, from 160 crops: 4 units per crop below 768 crops, 2 below 1536, 1 from there
    Fused('pool_rows', 'conv', (64, 32), [L((64, 32), 3, 32, 32, act=ACT_ELU, pool=True)], (160, 161, 768, 1536), (OPK_POOL_ROWS,), 159, wg_pool_rows),
    Fused('pool_rows_stem', 'stempool', (64, 32), [None, L((64, 32), 3, 32, 32, act=ACT_ELU, pool=True)], (160, 161, 768, 1536),
          (OPK_FOLDED, OPK_POOL_ROWS_STEM), 159, wg_pool_rows),
    # ---- SSD f16
    Fused('dwpw_rows_5x7', 'dwpw', (5, 7), [], (96, 97), (OPK_DWPW_ROWS,), 95, wg_tasks(lambda n: 2 * _parts(n, 2, 5, 3))),
    Fused('dwpw_rows_6x13', 'dwpw', (6, 13), [], (96, 97), (OPK_DWPW_ROWS,), 95, wg_tasks(lambda n: 3 * _parts(n, 3, 6, 3))),      # DR_SW = 6: two strips and a third one column wide
    Fused('dwpw_rows_75x75', 'dwpw', (75, 75), [], (96,), (OPK_DWPW_ROWS,), 95, wg_tasks(lambda n: 13 * _parts(n, 13, 75, 3)),
          ref_crops=(0, 1, 2, 47, -2, -1)),      # 5 625 pixels x 128 x 128 a crop: every crop's bits are still compared with the dwpw_k run
    Fused('ssd_front_12x20', 'ssdfront', (12, 20), [], (16, 17), (OPK_FOLDED, OPK_SSD_FRONT), 15, wg_tasks(lambda n: _parts(n, 1, 6, 2))),
    Fused('ssd_front_10x64', 'ssdfront', (10, 64), [], (16, 17), (OPK_FOLDED, OPK_SSD_FRONT), 15, wg_tasks(lambda n: 2 * _parts(n, 2, 5, 2))),   # SF_SW = 30: 32 columns = 30 + 2
    Fused('ssd_front_300x300', 'ssdfront', (300, 300), [], (16,), (OPK_FOLDED, OPK_SSD_FRONT), 15, wg_tasks(lambda n: 5 * _parts(n, 5, 150, 2)),
          ref_crops=(0, 1, 2, 7, -1)),
    # ---- the front of the 128 x 64 / 256 x 128 encoders as one launch (DD_STEM_WIDE=1, read on every forward), from 64 crops.  6 rows are the
    # fewest stem_wide_geometry takes: two pooled rows for four units a group, two of which have no row -- the kernel stores inside its rounds only
    Fused('stem_wide_6x64', 'stemwide', (6, 64), [None, L((6, 64), 3, 32, 32, act=ACT_ELU)], (64, 65, 257), (OPK_FOLDED, OPK_FOLDED, OPK_STEM_WIDE), 63,
          wg_stem_wide(64), env={'DD_STEM_WIDE': '1'}),
    Fused('stem_wide_8x128', 'stemwide', (8, 128), [None, L((8, 128), 3, 32, 32, act=ACT_ELU)], (64, 65, 257), (OPK_FOLDED, OPK_FOLDED, OPK_STEM_WIDE), 63,
          wg_stem_wide(128), env={'DD_STEM_WIDE': '1'}),
    # ---- conv_ws_dw_k: pointwise 256 -> C (ReLU6, hinted) + the next block's depthwise layer.  512 workgroups are 512 / (C / 128) workers of whole
    # frames and ws_dw_fusable wants them balanced: with C = 128 (512 workers) 256 and 384 frames are refused and 512 fuse; with C = 512 (128
    # workers) 256 and 384 frames fuse (2 and 3 frames a worker) and 200 are refused.  Refused: conv_ws_k and dwconv3_k, the same reference.
    Fused('ws_dw_c512_10x10', 'wsdw', (10, 10), [L((10, 10), 1, 256, 512, pad=0, act=ACT_RELU6)], (256, 384), (OPK_FOLDED, OPK_WS_DW), 159, wg_ws_dw(128),
          ref_crops=tuple(range(32)) + (127, 128, 129) + tuple(range(-32, 0))),
    Fused('ws_dw_c512_19x19', 'wsdw', (19, 19), [L((19, 19), 1, 256, 512, pad=0, act=ACT_RELU6)], (256, 384), (OPK_FOLDED, OPK_WS_DW), 159, wg_ws_dw(128),
          ref_crops=(0, 1, 2, 3, 127, 128, 129, -3, -2, -1)),      # 361 pixels x 256 x 512 a frame: every frame's bits are still compared with the two-launch run
    Fused('ws_dw_c128_10x10', 'wsdw', (10, 10), [L((10, 10), 1, 256, 128, pad=0, act=ACT_RELU6)], (512,), (OPK_FOLDED, OPK_WS_DW), 159, wg_ws_dw(512)),
    Fused('ws_dw_refused_c128_10x10', 'wsdw', (10, 10), [L((10, 10), 1, 256, 128, pad=0, act=ACT_RELU6)], (256, 384), (OPK_CONV_WS, OPK_DEFAULT), 159, wg_ws_dw(512)),
    Fused('ws_dw_refused_c512_10x10', 'wsdw', (10, 10), [L((10, 10), 1, 256, 512, pad=0, act=ACT_RELU6)], (200,), (OPK_CONV_WS, OPK_DEFAULT), 159, wg_ws_dw(128),
          ref_crops=tuple(range(32)) + (99, 100, 101) + tuple(range(-32, 0))),
    # ---- heights the matchers take (or took) that no network runs
    # res_unit_fusable: any H with W = 15.  res_unit_rows_k guards every row it fills, computes and stores by y < H: one row is handled
    Fused('res_unit_h1', 'unit_self', (1, 15), [L((1, 15), 3, 32, 32, act=ACT_ELU), L((1, 15), 3, 32, 32, res=True, dst2=True)], (512, 513, 2049),
          (OPK_FOLDED, OPK_RES_UNIT), 511, wg_wave4),
    Fused('res_unit_raw_sep_h1', 'unit', (1, 15), [L((1, 15), 3, 32, 32, act=ACT_ELU), L((1, 15), 3, 32, 32, res=True, dst2=True)], (512, 513, 2049),
          (OPK_FOLDED, OPK_RES_UNIT), 511, wg_wave4),
    # pool_rows_fusable took any even H; conv3x3_pool_rows_k stores a unit's last pooled row whether or not the unit has one, so with fewer pooled
    # rows than units (H < 10) it wrote an unset row in front of the crop's tensor: the matcher now wants four pooled rows and these run tiled
    Fused('pool_h4_generic', 'conv', (4, 32), [L((4, 32), 3, 32, 32, act=ACT_ELU, pool=True)], (160,), (OPK_DEFAULT,), None, wg_pool_rows),
    Fused('pool_h8_stem_generic', 'stempool', (8, 32), [None, L((8, 32), 3, 32, 32, act=ACT_ELU, pool=True)], (160, 768), (OPK_DEFAULT, OPK_DEFAULT), None, wg_pool_rows),
    Fused('pool_rows_h10', 'conv', (10, 32), [L((10, 32), 3, 32, 32, act=ACT_ELU, pool=True)], (160, 161), (OPK_POOL_ROWS,), 159, wg_pool_rows),
    # c64_rows_eligible took any even H; the 11-slot ring of conv3x3_c64_rows_k holds three rounds of look-ahead only if at most one of them opens
    # an image (H >= 6): the matcher now says so and 4 and 2 rows run on conv_glds_k (counts at which the engine does not split K)
    Fused('c64_h4_generic', 'conv', (4, 8), [L((4, 8), 3, 64, 64, act=ACT_ELU)], (1025,), (OPK_DEFAULT,), None, wg_wave2),
    Fused('c64_h2_generic', 'conv', (2, 8), [L((2, 8), 3, 64, 64, res=True, dst2=True)], (2049,), (OPK_DEFAULT,), None, wg_wave2),
    Fused('c64_rows_h6', 'conv', (6, 8), [L((6, 8), 3, 64, 64, res=True, dst2=True)], ROW_COUNTS, (OPK_C64_ROWS,), 511, wg_wave2),
]
BY_NAME = {c.name: c for c in CASES}
PARAMS = [(c, n) for c in CASES for n in c.counts]
IDS = ['%s-%d' % (c.name, n) for c, n in PARAMS]


# ---------------------------------------------------------------------------------------------- seeded weights of the ops that are no Conv
def stem_weights(stride, act, seed=41):
    rng = np.random.default_rng([seed, stride])
    g = C.pre_gain(act) / 3.0
    w = R.f16(g * rng.standard_normal((3, 3, 3, 32))).astype(np.float32)
    return w, (0.5 * C.pre_gain(act) * rng.standard_normal(32)).astype(np.float32)


def dwpw_weights(c, cout, seed=43):
    """As tests/test_gpu_net_ops.py::test_dwpw (ReLU6 both)."""
    dw_w, dw_b = C.dw_weights(c, ACT_RELU6)
    rng = np.random.default_rng([seed, c, cout])
    pw = R.f16(C.pre_gain(ACT_RELU6) / np.sqrt(c) / 3.0 * rng.standard_normal((c, cout))).astype(np.float32)
    return dw_w, dw_b, pw, (0.5 * C.pre_gain(ACT_RELU6) * rng.standard_normal(cout)).astype(np.float32)


MEAN, SCALE = 127.5, 1.0 / 127.5


# ---------------------------------------------------------------------------------------------- inputs
def images(case, n):
    """net_op_cases.images with crop 1 all 0 and crop 2 all 255; at the case's largest count the last crop of workgroup 0 and of the last
    workgroup are all 255 as well (a ring that serves a stale slot then shows)."""
    x = C.images(n, case.H, case.W, seed=51)
    if n > 1:
        x[1] = 0
    if n > 2:
        x[2] = 255
    if n == max(case.counts) and n > 3:
        wg = case.wg(n)
        for g in (0, int(wg.max())):
            own = np.flatnonzero(wg == g)         # (conv_ws_dw_k with fewer frames than workers: worker 0 has none)
            if len(own):
                x[int(own[-1])] = 255
    return x


def cpu_inputs(case, img):
    """The feeder tensors `build` makes, emulated on the CPU (net_op_cases.emulate_feeder): inputs of the same kind for the CPU tests."""
    ly = case.layers
    f = lambda c, seed: C.emulate_feeder(img, *C.feeder_weights(c, seed))      # noqa: E731
    if case.kind == 'conv':
        return dict(x=f(ly[0].cin, 1), **({'res': f(ly[0].cout, 2)} if ly[0].res else {}))
    if case.kind in ('s2proj', 'projblock'):
        return dict(x=f(ly[0].cin, 1), x2=f(ly[1].cin, 2))
    if case.kind in ('unit', 'unit_self'):
        x = f(ly[0].cin, 1)
        return dict(x=x, res=x if case.kind == 'unit_self' else f(ly[1].cout, 2))
    if case.kind == 'pair':
        return dict(x=f(32, 1))
    if case.kind == 'dwpw':
        return dict(x=f(128, 1))
    if case.kind == 'wsdw':
        return dict(x=f(ly[0].cin, 1))
    return {}


def pick(case, n):
    """The crops the reference is computed for: all of them up to 2 CU + 1 (mars_ws128_k: always all); above that 0, 1, 2, CU - 1, CU, CU + 1, the
    last CU + 2 and every crop of workgroup 0."""
    if case.ref_crops is not None:        # a map so large that the float64 reference of every crop takes minutes: the stated crops only
        return np.unique(np.concatenate([np.asarray(case.ref_crops) % n, np.flatnonzero(case.wg(n) == 0)]))
    if n <= 2 * CU + 1 or case.chunk is None:
        return np.arange(n)
    return np.unique(np.concatenate([[0, 1, 2, CU - 1, CU, CU + 1], np.arange(n - CU - 2, n), np.flatnonzero(case.wg(n) == 0)]))


# ---------------------------------------------------------------------------------------------- programs
class Built:
    def __init__(self):
        self.inputs, self.outs, self.hidden, self.mids, self.first_op = {}, {}, [], None, 0


def build(case, rig):
    """Adds the case's program to rig.p.  Returns Built: inputs name -> feeder tensor, outs name -> tensor the launch writes, hidden = tensors
    the fused launch keeps on the chip (reading them is refused), first_op = index of the first op under test."""
    nets, p, b, ly = rig.nets, rig.p, Built(), case.layers

    def conv(src, l, res=-1, hint=0, with_dst2=None, name=None):
        kw = {}
        if l.dst2 if with_dst2 is None else with_dst2:
            kw = dict(dst2=p.tensor(l.ho, l.wo, l.cout), aff2=l.aff2)
        t = p.conv(src, l.w, l.b, stride=l.stride, pad=l.pad, act=l.act, res=res, pool=l.pool, **kw)
        p.ops[-1][nets.HINT] = hint
        return (t, kw['dst2']) if kw else t

    if case.kind == 'conv':
        l = ly[0]
        b.inputs['x'] = rig.feeder(l.cin, 1)
        if l.res:
            b.inputs['res'] = rig.feeder(l.cout, 2)
        b.first_op = len(p.ops)
        r = conv(b.inputs['x'], l, res=b.inputs.get('res', -1))
        b.outs['out'], b.outs['out2'] = r if l.dst2 else (r, None)
    elif case.kind == 's2proj':
        b.inputs['x'], b.inputs['x2'] = rig.feeder(64, 1), rig.feeder(64, 2)
        b.first_op = len(p.ops)
        b.outs['out'] = conv(b.inputs['x'], ly[0], hint=nets.HINT_NEXT_IS_PROJ)
        b.outs['proj'] = conv(b.inputs['x2'], ly[1])
    elif case.kind in ('unit', 'unit_self'):
        b.inputs['x'] = rig.feeder(ly[0].cin, 1)
        b.inputs['res'] = b.inputs['x'] if case.kind == 'unit_self' else rig.feeder(ly[1].cout, 2)
        b.first_op = len(p.ops)
        h1 = conv(b.inputs['x'], ly[0], hint=nets.HINT_PAIR_MEMBER if ly[0].cin == 64 else nets.HINT_NEXT_ONLY)
        b.outs['out'], b.outs['out2'] = conv(h1, ly[1], res=b.inputs['res'])
        b.hidden = [h1]
    elif case.kind == 'pair':
        b.inputs['x'] = rig.feeder(32, 1)
        b.first_op = len(p.ops)
        h1 = conv(b.inputs['x'], ly[0], hint=nets.HINT_NEXT_ONLY)
        o1, o12 = conv(h1, ly[1], res=b.inputs['x'], hint=nets.HINT_HOLD_UNIT)
        h2 = conv(o12, ly[2], hint=nets.HINT_NEXT_ONLY)
        b.outs['out'], b.outs['out2'] = conv(h2, ly[3], res=o1)
        b.hidden = [h1, o1, o12, h2]
    elif case.kind == 'projblock':
        b.inputs['x'], b.inputs['x2'] = rig.feeder(32, 1), rig.feeder(32, 2)
        b.first_op = len(p.ops)
        h1 = conv(b.inputs['x'], ly[0], hint=nets.HINT_NEXT_IS_PROJ)
        sk = conv(b.inputs['x2'], ly[1], hint=nets.HINT_PAIR_MEMBER)
        b.outs['out'], b.outs['out2'] = conv(h1, ly[2], res=sk)
        b.hidden = [sk, h1]           # (in the order the reference meets them)
    elif case.kind in ('stempool', 'stemwide'):
        w0, b0 = stem_weights(1, ACT_ELU)
        b.first_op = len(p.ops)
        t = p.stem(w0, b0, 1, nets.ACT_ELU, swap_rb=True, mean=MEAN, scale=SCALE)
        p.ops[-1][nets.HINT] = nets.HINT_NEXT_ONLY
        if case.kind == 'stempool':
            b.outs['out'] = conv(t, ly[1])
            b.hidden = [t] if case.codes[0] == OPK_FOLDED else []
        else:                                # conv1_2 and the pool as ops of their own, as compile_mars writes them at widths 64 and 128
            c = conv(t, ly[1])
            b.outs['out'] = p.maxpool(c, 3, 2, 0)
            b.hidden = [t, c]
        b.mids = [t]
    elif case.kind == 'wsdw':
        l = ly[0]
        b.inputs['x'] = rig.feeder(l.cin, 1)
        b.first_op = len(p.ops)
        t = conv(b.inputs['x'], l, hint=nets.HINT_NEXT_ONLY)
        dw_w, dw_b = C.dw_weights(l.cout, ACT_RELU6)
        b.outs['out'] = p.dwconv(t, dw_w, dw_b, 1, nets.ACT_RELU6)
        b.hidden = [t] if case.codes[0] == OPK_FOLDED else []
        b.mids = [t]
    elif case.kind == 'ssdfront':
        w0, b0 = stem_weights(2, ACT_RELU6)
        dw_w, dw_b, pw, pw_b = dwpw_weights(32, 64)
        b.first_op = len(p.ops)
        t = p.stem(w0, b0, 2, nets.ACT_RELU6, swap_rb=False, mean=MEAN, scale=SCALE)
        p.ops[-1][nets.HINT] = nets.HINT_NEXT_ONLY
        b.outs['out'] = p.dwpw(t, dw_w, dw_b, 1, nets.ACT_RELU6, pw.reshape(1, 1, 32, 64), pw_b, nets.ACT_RELU6)
        assert p.ops[-1][0] == nets.OP_DWPW
        b.hidden = [t]
    elif case.kind == 'dwpw':
        dw_w, dw_b, pw, pw_b = dwpw_weights(128, 128)
        b.inputs['x'] = rig.feeder(128, 1)
        b.first_op = len(p.ops)
        b.outs['out'] = p.dwpw(b.inputs['x'], dw_w, dw_b, 1, nets.ACT_RELU6, pw.reshape(1, 1, 128, 128), pw_b, nets.ACT_RELU6)
        assert p.ops[-1][0] == nets.OP_DWPW
    else:
        raise ValueError(case.kind)
    b.outs = {k: v for k, v in b.outs.items() if v is not None}
    for t in list(b.outs.values()):
        p.keep.add(t)
    if b.mids is None:
        b.mids = list(b.hidden)           # the tensors between the layers, in the order the reference meets them
    return b


# ---------------------------------------------------------------------------------------------- references
def one_layer(l, x, res=None):
    """net_op_cases.conv_reference of one layer (epilogue, second output, fused pool), with the stages net_op_ref.hook names."""
    x, w = np.asarray(x, np.float64)[..., :l.cin], R.f16(l.w)
    s, S = R.conv(x, w, l.b, l.stride, l.pad_t, l.pad_l, l.ho, l.wo)
    s = R.hook('last.s', s, x=x, w=w, b=l.b, geom=(l.stride, l.pad_t, l.pad_l, l.ho, l.wo), dw=False)
    r = C.finish_reference(l, s, S, R.hook('res', res), l.aff2)
    return {k: (R.hook('pool', v[0]), v[1]) for k, v in r.items()} if l.pool else r


def reference(case, inp, img=None):
    """{name: (want, bound)} of every tensor the launch writes, from the f16 tensors `inp` the ops read (float64; `img`: the u8 crops, for the cases
    whose first layer reads them)."""
    ly = case.layers
    if case.kind == 'conv':
        return one_layer(ly[0], inp['x'], inp.get('res'))
    if case.kind == 's2proj':
        return {'out': one_layer(ly[0], inp['x'])['out'], 'proj': one_layer(ly[1], inp['x2'])['out']}
    if case.kind in ('unit', 'unit_self'):
        return R.res_unit(inp['x'][..., :ly[0].cin], inp['res'], _a(ly[0]), (R.f16(ly[1].w), ly[1].b), ly[1].aff2)
    if case.kind == 'pair':
        return R.res_pair(inp['x'], _a(ly[0]), (R.f16(ly[1].w), ly[1].b), ly[1].aff2, _a(ly[2]), (R.f16(ly[3].w), ly[3].b), ly[3].aff2)
    if case.kind == 'projblock':
        return R.proj_block(inp['x'], inp['x2'], _a(ly[0]), (R.f16(ly[1].w), ly[1].b), (R.f16(ly[2].w), ly[2].b), ly[2].aff2)
    if case.kind == 'wsdw':
        dw_w, dw_b = C.dw_weights(ly[0].cout, ACT_RELU6)
        return {'out': R.pw_dw(inp['x'], R.f16(ly[0].w)[0, 0], ly[0].b, R.f16(dw_w), dw_b)}
    if case.kind in ('stempool', 'stemwide'):
        w0, b0 = stem_weights(1, ACT_ELU)
        return R.stem_conv_pool(img, w0, b0, True, MEAN, SCALE, R.f16(ly[1].w), ly[1].b)
    if case.kind == 'ssdfront':
        w0, b0 = stem_weights(2, ACT_RELU6)
        dw_w, dw_b, pw, pw_b = dwpw_weights(32, 64)
        return {'out': R.ssd_front(img, w0, b0, MEAN, SCALE, R.f16(dw_w), dw_b, R.f16(pw), pw_b)}
    if case.kind == 'dwpw':
        dw_w, dw_b, pw, pw_b = dwpw_weights(128, 128)
        return {'out': R.dwpw(inp['x'], R.f16(dw_w), dw_b, 1, 1, 1, case.H, case.W, ACT_RELU6, R.f16(pw), pw_b, ACT_RELU6)}
    raise ValueError(case.kind)
