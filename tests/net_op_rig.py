"""The program rig of tests/test_gpu_net_ops.py and tests/test_gpu_fused_ops.py."""
import net_op_cases as C


class Rig:
    """Program with in_h, in_w = H, W, an input op ((x - 127.5) / 127.5) and feeders; one forward on the seeded u8 batch (or on `img`)."""

    def __init__(self, H, W, n, seed=11, program_input=True, img=None):
        from deepdish_amd import nets
        self.nets, self.n = nets, n
        self.p = nets.Program(H, W)
        self.img = C.images(n, H, W, seed) if img is None else img
        self.t_in = self.p.input(swap_rb=False, mean=127.5, scale=1.0 / 127.5) if program_input else -1

    def feeder(self, c, wseed, stride=1, gain=1.0, bias=0.0, dst=None):
        w, b = C.feeder_weights(c, wseed, gain, bias)
        t = self.p.conv(self.t_in, w, b, stride=stride, pad=0, act=self.nets.ACT_NONE, dst=dst)
        self.p.keep.add(t)
        return t

    def run(self, out, max_batch=None):
        from deepdish_amd.engine import Net
        self.p.out_tensor = out
        self.net = Net(self.p, max_batch=max_batch or self.n)
        self.net.forward(self.img)
        return self

    def forward(self, img):
        """Another forward of the same engine (same max_batch, same split-K decisions) on fewer crops."""
        self.net.forward(img)
        return self

    def raw(self, t):
        return self.net.read(tensor=t)

    def read(self, t):
        import numpy as np
        return self.raw(t).astype(np.float64)

    def launches(self):
        from deepdish_amd.profile import net_op_launches
        return [int(c) for c in net_op_launches(self.net)]

    def kernel_of(self, op):
        from deepdish_amd.profile import net_op_launches, net_op_variants
        return int(net_op_launches(self.net)[op]), net_op_variants(self.net)[op]
