"""The one-op cases of tests/test_gpu_net_ops.py and tests/test_net_op_ref.py: shapes, seeded inputs and the kernel each conv case must reach.

A case is the smallest shape that reaches one branch of net_run_ops (csrc/nets.hip) or one tail of a kernel.  `variant` is what
dd_net_op_variants must report for the op -- (WM, WN, MI, NI, BK, mode, splitk), mode 0 / 1 / 2 = conv_glds_k general / pointwise / whole-tap
fill, 3 = conv_mfma_k -- and `opk` its dd_net_op_launches code; both are literals, written down from reading the dispatcher once, not
recomputed from a copy of its rules.  Here K = kh * kw * rup(cin, 8), bk = 32 if K <= 96 else 64, m = n * ho * wo.

Four rows of the case table this file was written from name conv_glds_k for 1x1 layers with 64 input channels.  Their K is 64, so by the rule
above they are bk = 32 layers and run on conv_mfma_k.  Those cases are kept as stated, with the variant they do reach, and each has a twin with
128 (or 104) input channels that reaches the conv_glds_k branch the row names (`twin of`).
"""
import numpy as np

from net_op_ref import ACT_NONE, ACT_RELU6, ACT_ELU, ACT_SILU, ACT_RELU, ACT_SIGMOID, ACTS, f16, rup, geometry

OPK_DEFAULT, OPK_CONV_WS = 0, 8
ACT_NAMES = {ACT_NONE: 'none', ACT_RELU6: 'relu6', ACT_ELU: 'elu', ACT_SILU: 'silu', ACT_RELU: 'relu', ACT_SIGMOID: 'sigmoid'}


class Conv:
    """One dense convolution case.  pad None = TF SAME, else symmetric.  epi: 'f16', 'f32' or 'f32aff' (EPI_F32 with post_aff).
    max_batch None = n.  cpu_n: images the CPU mutant test evaluates (the first ones of the same seeded batch)."""

    def __init__(self, name, hw, n, k, cin, cout, variant, stride=1, pad=None, act=ACT_NONE, res=False, dst2=False, epi='f16',
                 max_batch=None, opk=OPK_DEFAULT, pool=False):
        self.name, (self.H, self.W), self.n = name, hw, n
        self.kh, self.kw = (k, k) if isinstance(k, int) else k
        self.cin, self.cout, self.stride, self.pad, self.act = cin, cout, stride, pad, act
        self.res, self.dst2, self.epi, self.max_batch, self.variant, self.opk, self.pool = res, dst2, epi, max_batch or n, variant, opk, pool
        self.ho, self.wo, self.pad_t, self.pad_l = geometry(self.H, self.W, self.kh, self.kw, stride, pad)
        self.cin_pad, self.cout_pad = rup(cin, 8), rup(cout, 8)
        self.K = self.kh * self.kw * self.cin_pad
        self.bk = 32 if self.K <= 96 else 64
        self.kpad = rup(self.K, self.bk)
        self.splitk = variant[6] if variant else 1
        self.n_terms = self.kh * self.kw * cin
        self.cpu_n = min(n, 3)

    def __repr__(self):
        return self.name

    def with_(self, name, **kw):
        d = dict(hw=(self.H, self.W), n=self.n, k=(self.kh, self.kw), cin=self.cin, cout=self.cout, variant=self.variant, stride=self.stride,
                 pad=self.pad, act=self.act, res=self.res, dst2=self.dst2, epi=self.epi, max_batch=self.max_batch, opk=self.opk, pool=self.pool)
        d.update(kw)
        return Conv(name, **d)


M32, M64 = (4, 1, 1, 2, 32, 3, 1), (2, 2, 2, 2, 32, 3, 1)          # conv_mfma_k<4,1,1,2,32> / <2,2,2,2,32>


def G(tile, mode, splitk=1):
    return tile + (64, mode, splitk)


T32, T64 = (4, 1, 1, 2), (2, 2, 2, 2)

CONV_CASES = [
    # conv_mfma_k<4,1,1,2,32>: cout_pad <= 32, bk 32; m = 105, no multiple of 128
    Conv('mfma32_3x3_c8_24', (7, 5), 3, 3, 8, 24, M32, act=ACT_RELU6),
    Conv('mfma32_1x1_c3_32', (7, 5), 3, 1, 3, 32, M32, act=ACT_SILU),
    Conv('mfma32_1x3_c16_20', (7, 5), 3, (1, 3), 16, 20, M32, act=ACT_ELU),
    # conv_mfma_k<2,2,2,2,32>: cout_pad 72, no multiple of 64
    Conv('mfma64_1x1_c16_72', (9, 7), 1, 1, 16, 72, M64, act=ACT_RELU6),
    # conv_glds_k mode 1 (pointwise)
    Conv('pw_c128_32', (7, 5), 3, 1, 128, 32, G(T32, 1), act=ACT_SILU),
    Conv('pw_c64_200', (7, 5), 3, 1, 64, 200, M64, act=ACT_RELU6),                      # as stated: K = 64 is a bk-32 layer
    Conv('pw_c128_200', (7, 5), 3, 1, 128, 200, G(T64, 1), act=ACT_RELU6),              # twin of pw_c64_200: <2,2,2,2,64> pointwise
    # mode 2 (whole taps): every such layer on these small maps is also split along K (9 steps -> 5 + 4)
    Conv('taps_c64_24', (7, 5), 3, 3, 64, 24, G(T32, 2, 2), act=ACT_ELU),
    Conv('taps_c64_136', (7, 5), 3, 3, 64, 136, G(T64, 2, 2), act=ACT_SILU),
    Conv('taps_s2same_c64_24', (8, 6), 3, 3, 64, 24, G(T32, 2, 2), stride=2, act=ACT_RELU6),       # asymmetric pad: 0 before, 1 behind
    Conv('taps_s2pad1_c64_136', (7, 5), 3, 3, 64, 136, G(T64, 2, 2), stride=2, pad=1, act=ACT_SILU),
    Conv('taps_c64_24_unsplit', (7, 5), 3, 3, 64, 24, G(T32, 2), act=ACT_ELU, max_batch=600),      # an engine sized for 600 images does not split
    Conv('taps_c64_136_unsplit', (7, 5), 3, 3, 64, 136, G(T64, 2), act=ACT_SILU, max_batch=600),
    Conv('taps_s2same_c64_24_unsplit', (8, 6), 3, 3, 64, 24, G(T32, 2), stride=2, act=ACT_RELU6, max_batch=1500),
    # mode 0 (general fill)
    Conv('gen_s2_c16_32', (8, 6), 3, 3, 16, 32, G(T32, 0), stride=2, act=ACT_RELU6),               # K 144, kpad 192
    Conv('gen_c40_72', (7, 5), 3, 3, 40, 72, G(T64, 0), act=ACT_ELU),                            # cin % 64 != 0
    Conv('gen_5x5_c8_40', (7, 5), 3, 5, 8, 40, G(T64, 0), pad=2, act=ACT_SILU),                  # K 200, kpad 256: last step a quarter full
    Conv('pw_s2_c64_128', (7, 5), 3, 1, 64, 128, M64, stride=2, act=ACT_RELU6),                  # as stated: K = 64 is a bk-32 layer
    Conv('pw_s2_c104_128', (7, 5), 3, 1, 104, 128, G(T64, 0), stride=2, act=ACT_RELU6),          # twin: 1x1 stride 2 through the general fill
    Conv('pw_s2_c128_128', (7, 5), 3, 1, 128, 128, G(T64, 2), stride=2, act=ACT_RELU6),          # ... and through the whole-tap fill (cin % 64 == 0)
    # tiles picked by m, 19 x 19; in every one m is no multiple of the tile.  As stated (cin 64: conv_mfma_k at large m) ...
    Conv('m4332_c64_128', (19, 19), 12, 1, 64, 128, M64, act=ACT_RELU6),
    Conv('m16606_c64_128', (19, 19), 46, 1, 64, 128, M64, act=ACT_RELU6),
    Conv('m16606_c64_64', (19, 19), 46, 1, 64, 64, M64, act=ACT_SILU),
    Conv('m16606_c64_32', (19, 19), 46, 1, 64, 32, M32, act=ACT_ELU),
    Conv('m76893_c64_128', (19, 19), 213, 1, 64, 128, M64, act=ACT_RELU6),
    # ... and their twins with cin 128, which reach the conv_glds_k tiles the row names
    Conv('m4332_c128_128', (19, 19), 12, 1, 128, 128, G((2, 2, 2, 4), 1), act=ACT_RELU6),
    Conv('m16606_c128_128', (19, 19), 46, 1, 128, 128, G((4, 2, 2, 4), 1), act=ACT_RELU6),
    Conv('m16606_c128_64', (19, 19), 46, 1, 128, 64, G((4, 2, 2, 2), 1), act=ACT_SILU),
    Conv('m16606_c128_32', (19, 19), 46, 1, 128, 32, G((4, 1, 2, 2), 1), act=ACT_ELU),
    Conv('m76893_c128_128', (19, 19), 213, 1, 128, 128, G((4, 2, 3, 4), 1), act=ACT_RELU6),       # 600 tiles of 128 = two rounds, 400 of 192 = one
    # split-K: 9 steps -> 5 + 4; 18 steps -> 5 + 5 + 5 + 3
    Conv('splitk2', (5, 5), 2, 3, 64, 72, G(T64, 2, 2), act=ACT_ELU),
    Conv('splitk2_res_dst2', (5, 5), 2, 3, 64, 72, G(T64, 2, 2), res=True, dst2=True),
    Conv('splitk2_f32aff', (5, 5), 2, 3, 64, 72, G(T64, 2, 2), act=ACT_ELU, epi='f32aff'),
    Conv('splitk4', (5, 5), 2, 3, 128, 72, G(T64, 2, 4), act=ACT_SILU),
    Conv('splitk4_res_dst2', (5, 5), 2, 3, 128, 72, G(T64, 2, 4), res=True, dst2=True),
    Conv('splitk4_f32aff', (5, 5), 2, 3, 128, 72, G(T64, 2, 4), act=ACT_ELU, epi='f32aff'),
    # conv_ws_k: m = 19 360
    Conv('ws_c256_128_relu6', (11, 11), 160, 1, 256, 128, None, act=ACT_RELU6, opk=OPK_CONV_WS),
    Conv('ws_c256_128_silu', (11, 11), 160, 1, 256, 128, None, act=ACT_SILU, opk=OPK_CONV_WS),
    Conv('ws_c512_256_relu6', (11, 11), 160, 1, 512, 256, None, act=ACT_RELU6, opk=OPK_CONV_WS),
    Conv('ws_c512_256_silu', (11, 11), 160, 1, 512, 256, None, act=ACT_SILU, opk=OPK_CONV_WS),
    # conv3x3_rw_k (3x3 stride 1 pad 1, 32 -> 32): one tile, and several uneven ones
    Conv('rw_5x7', (5, 7), 2, 3, 32, 32, None, act=ACT_ELU),
    Conv('rw_5x7_res', (5, 7), 2, 3, 32, 32, None, act=ACT_SILU, res=True),
    Conv('rw_5x7_res_dst2', (5, 7), 2, 3, 32, 32, None, res=True, dst2=True),
    Conv('rw_37x33', (37, 33), 2, 3, 32, 32, None, act=ACT_ELU),
    Conv('rw_37x33_res', (37, 33), 2, 3, 32, 32, None, act=ACT_SILU, res=True),
    Conv('rw_37x33_res_dst2', (37, 33), 2, 3, 32, 32, None, res=True, dst2=True),
    Conv('rw_37x33_pool', (37, 33), 2, 3, 32, 32, None, act=ACT_ELU, pool=True),
    Conv('rw_6x6_pool', (6, 6), 2, 3, 32, 32, None, act=ACT_ELU, pool=True),                      # pooled 2 x 2
]


def _flavours(tag, base, f16_out=True):
    """Every ACT_*, res, res + dst2 / aff2 (f16 outputs) or EPI_F32 with and without post_aff on one path; cout = 8 k + 5."""
    out = [base.with_('%s_%s' % (tag, ACT_NAMES[a]), act=a, epi='f16' if f16_out else 'f32') for a in ACTS]
    if f16_out:
        out += [base.with_(tag + '_silu_res', act=ACT_SILU, res=True), base.with_(tag + '_none_res_dst2', act=ACT_NONE, res=True, dst2=True),
                base.with_(tag + '_elu_res_dst2', act=ACT_ELU, res=True, dst2=True)]
    else:
        out += [base.with_(tag + '_f32_silu_res', act=ACT_SILU, res=True, epi='f32'), base.with_(tag + '_f32aff_elu', act=ACT_ELU, epi='f32aff')]
    return out


EPILOGUE_CASES = (
    _flavours('epi_mfma', Conv('', (7, 5), 3, 3, 8, 21, M32))                                     # conv_finish_rows (staged through LDS)
    + _flavours('epi_mfma_f32', Conv('', (7, 5), 3, 3, 8, 21, M32), f16_out=False)                # conv_epilogue, four channels per lane
    + _flavours('epi_glds_direct', Conv('', (7, 5), 3, 1, 128, 29, G(T32, 1)))                   # conv_finish_direct
    + _flavours('epi_glds_staged', Conv('', (7, 5), 3, 1, 128, 29, G(T32, 1)), f16_out=False)    # conv_finish behind conv_glds_k (no f16 direct store)
    + _flavours('epi_splitk', Conv('', (5, 5), 2, 3, 64, 69, G(T64, 2, 2)))                      # conv_splitk_finish_k
    + _flavours('epi_splitk_f32', Conv('', (5, 5), 2, 3, 64, 69, G(T64, 2, 2)), f16_out=False))

ALL_CONV_CASES = CONV_CASES + EPILOGUE_CASES


class Dw:
    def __init__(self, hw, c, stride, act, n=3):
        (self.H, self.W), self.c, self.stride, self.act, self.n = hw, c, stride, act, n
        self.ho, self.wo, self.pad_t, self.pad_l = geometry(self.H, self.W, 3, 3, stride, None)
        self.name = 'dw_%dx%d_c%d_s%d_%s' % (hw[0], hw[1], c, stride, ACT_NAMES[act])
        self.cpu_n = n

    def __repr__(self):
        return self.name


# stride 1 (two-row form) on 5x7 and 6x9: odd ho, wo % 4 != 0; stride 2 SAME on 8x6 (asymmetric) and 7x5
DW_CASES = [Dw(hw, c, s, a) for c in (8, 40) for (hw, s) in (((5, 7), 1), ((6, 9), 1), ((8, 6), 2), ((7, 5), 2))
            for a in (ACT_RELU6, ACT_SILU, ACT_NONE)]

DWPW_SHAPES = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2)]         # nets.Program.DWPW_SHAPES, with the map each stride runs on
DWPW_MAPS = {1: (6, 10), 2: (7, 9)}


# ---------------------------------------------------------------------------------------------- seeded inputs
def images(n, H, W, seed):
    """u8 batch; every image is drawn on its own, so the first k images of a larger batch are the batch of k.  Pixels 0 and 255 are present."""
    x = np.stack([np.random.default_rng([seed, i]).integers(0, 256, (H, W, 3), dtype=np.uint8) for i in range(n)])
    x[0, 0, 0], x[0, 0, 1 % W] = 0, 255
    return x


def feeder_weights(c, seed, gain=1.0, bias=0.0):
    """1x1 feeder 3 -> c on pixels normalised to [-1, 1] (variance 1/3 each): weights N(0, gain^2) make values of order `gain` with both
    signs (bias < 0 and a small gain: all negative).  f16-exact weights."""
    rng = np.random.default_rng([seed, c, 77])
    w = f16(gain * rng.standard_normal((1, 1, 3, c))).astype(np.float32)
    b = (bias + 0.5 * gain * rng.standard_normal(c)).astype(np.float32)
    return w, b


def emulate_feeder(img, w, b, stride=1):
    """What the input op + feeder produce, on the CPU: f16 of (x - 127.5) / 127.5, then the 1x1 layer, f16 again.  (The GPU tests read the
    feeder's own bits back instead; this is for the CPU tests, which need inputs of the same kind.)"""
    x = f16((img.astype(np.float64) - 127.5) * float(np.float32(1 / 127.5)))[:, ::stride, ::stride]
    return f16(x @ np.asarray(w, np.float64)[0, 0] + np.asarray(b, np.float64))


def pre_gain(act):
    """Scale of the pre-activation values: ReLU6 needs >= 5 % of them on each side of 6 as well as of 0."""
    return 4.0 if act == ACT_RELU6 else 2.0


def conv_weights(case, seed=5):
    rng = np.random.default_rng([seed, case.kh, case.kw, case.cin, case.cout])
    g = pre_gain(case.act) / np.sqrt(case.n_terms)
    w = f16(g * rng.standard_normal((case.kh, case.kw, case.cin, case.cout))).astype(np.float32)
    b = (0.5 * pre_gain(case.act) * rng.standard_normal(case.cout)).astype(np.float32)
    aff2 = (rng.uniform(0.5, 1.5, case.cout).astype(np.float32) * rng.choice([-1.0, 1.0], case.cout).astype(np.float32),
            (0.3 * rng.standard_normal(case.cout)).astype(np.float32))
    return w, b, aff2


def dw_weights(c, act, seed=6):
    rng = np.random.default_rng([seed, c])
    g = pre_gain(act) / 3.0
    return f16(g * rng.standard_normal((3, 3, c))).astype(np.float32), (0.5 * pre_gain(act) * rng.standard_normal(c)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the other ops' geometries
POOL_CASES = [((7, 5), 3, 2, 0), ((7, 5), 3, 2, 1), ((8, 8), 3, 2, 0), ((8, 8), 3, 2, 1), ((7, 5), 5, 1, 2), ((8, 8), 5, 1, 2)]     # (map, k, stride, pad)
CASCADE_CASES = [((7, 5), 32), ((7, 5), 64), ((20, 20), 32), ((20, 20), 64)]                                                    # k = 5, n = 3
UPSAMPLE_CASES = [((3, 5), 8), ((3, 5), 40)]
INPUT_NORMS = [(0.0, 1.0), (127.5, 1.0 / 127.5), (0.0, 1.0 / 255.0)]
INPUT_CASES = ([dict(swap_rb=s, mean=m, scale=sc, s2d=False, c_pad=cp) for s in (False, True) for (m, sc) in INPUT_NORMS for cp in (0, 8, 32)]
               + [dict(swap_rb=s, mean=m, scale=sc, s2d=True, c_pad=cp) for s in (False, True) for (m, sc) in INPUT_NORMS for cp in (0, 32)])    # s2d: cs 16 and 32
INPUT_MAP = (6, 10)
STEM_CASES = [dict(hw=hw, stride=st, cout=co, swap_rb=sw, act=a, mean=m, scale=sc)
              for (hw, st) in (((7, 5), 1), ((8, 6), 2), ((7, 5), 2), ((8, 6), 1))
              for (co, sw, a, m, sc) in ((32, True, ACT_ELU, 0.0, 1.0 / 128), (24, False, ACT_RELU6, 127.5, 1.0 / 127.5))]


def conv_reference(case, x, res=None, weights=None):
    """{'out': (want, bound)[, 'out2': ...]} of a Conv case from the f16 activations x (and residual) the op read, all channels up to cout_pad;
    also returns the pre-activation sums."""
    import net_op_ref as R
    w, b, aff2 = weights if weights is not None else conv_weights(case)
    s, S = R.conv(np.asarray(x, np.float64)[..., :case.cin], f16(w), b, case.stride, case.pad_t, case.pad_l, case.ho, case.wo)
    return finish_reference(case, s, S, res, aff2), s


def finish_reference(case, s, S, res, aff2):
    import net_op_ref as R
    r = R.epilogue(s, S, case.n_terms, case.cout_pad, case.act, case.splitk, res=res[..., :case.cout] if res is not None else None,
                   aff2=aff2 if case.dst2 else None, f32=case.epi != 'f16', post_aff=aff2 if case.epi == 'f32aff' else None)
    if case.pool:      # 3x3 stride-2 VALID max pool of the f16 tile: a maximum moves by no more than its operands do
        r = {k: (R.maxpool(v[0], 3, 2, 0), R.maxpool(v[1], 3, 2, 0)) for k, v in r.items()}
    return r
