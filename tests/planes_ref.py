"""The depth / alpha planes (FR_FLAG_DEPTH_ALPHA) from the CPU oracle alone: nothing here runs the code under test.

The oracle has no planes of its own.  A frame of the same Gaussians with colors_precomp = (z, 0, 0) (z: the float32 view-space
depth of every mean) over bg = (0, 1, 0) renders the depth plane in colour channel 0 — sum of z alpha T, summed like a colour
channel in the same order — and 1 - alpha in channel 1 (the background's share: T_final).  Gradients of
<gC, C> + <gD, D> + <gA, A> are those of the plain frame under gC plus those of that composite frame under (gD, -gA, 0), with
dL/dz (the composite frame's dL_dcolors[:, 0]) carried into the means through the view matrix.

The bound of every gradient array is max(1e-4, NOISE_K x floor): the floor is the rel-L2, against the default sum, of the same
sum from the oracle's backward in two other float orders (one of them with contractions), as `_check_backward` of
tests/test_gpu_parity.py measures it — on the reference only, never on the result that is checked."""
import numpy as np

from oracle import oracle
from tests import util
from tests.test_gpu_parity import NOISE_K


def view_depth(s):
    """z = m[2] x + m[6] y + m[10] z + m[14] in float32 (row-major "transposed" view matrix); -> (z, m)."""
    m = s.camera.world_view_transform.astype(np.float32).reshape(-1)
    z = (s.means3D[:, 0] * m[2] + s.means3D[:, 1] * m[6] + s.means3D[:, 2] * m[10] + m[14]).astype(np.float32)
    return z, m


def composite_forward(s, z):
    c = s.camera
    return oracle.forward(bg=np.array([0.0, 1.0, 0.0], np.float32), means3D=s.means3D, opacities=s.opacities,
                          viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, campos=c.camera_center,
                          tanfovx=c.tanfovx, tanfovy=c.tanfovy, H=c.image_height, W=c.image_width, sh_degree=s.sh_degree,
                          colors_precomp=np.stack([z, np.zeros_like(z), np.zeros_like(z)], 1), scales=s.scales, rotations=s.rotations)


class PlanesRef:
    """The oracle's plain frame `o`, its composite frame `comp`, the expected planes and the expected gradients of a scene."""

    def __init__(self, s):
        self.s = s
        self.H, self.W = s.camera.image_height, s.camera.image_width
        self.z, self.m = view_depth(s)
        self.o = util.oracle_forward(s)
        self.comp = composite_forward(s, self.z)
        assert np.array_equal(self.comp.radii, self.o.radii)
        self.depth = self.comp.color[0]
        self.alpha = np.float32(1) - self.comp.color[1]

    def sum_gradients(self, gC, g_comp):
        """oracle.backward(o, gC) + oracle.backward(comp, g_comp), dL/dz through z, in the oracle's current float order."""
        b_plain = oracle.backward(self.o, gC)
        b_comp = oracle.backward(self.comp, g_comp)
        dz = b_comp.dL_dcolors[:, 0:1]
        want = {}
        for k in util.GRAD_NAMES:
            a, b = getattr(b_plain, k), getattr(b_comp, k)
            if k in ("dL_dcolors", "dL_dsh"):
                want[k] = a                                   # (the composite colours are not the frame's parameters)
            elif k == "dL_dmeans3D":
                want[k] = a + b + dz * self.m[[2, 6, 10]].reshape(1, 3)
            else:
                want[k] = a + b
        return want

    def gradients(self, gC, gD, gA):
        """Expected gradients of <gC, C> + <gD, D> + <gA, A> (a None upstream is a zero plane) ->
        ({array: expected}, {array: float-order floor}, {array: bound})."""
        zero = np.zeros((self.H, self.W), np.float32)
        gC = np.zeros((3, self.H, self.W), np.float32) if gC is None else gC
        gD, gA = zero if gD is None else gD, zero if gA is None else gA
        g_comp = np.ascontiguousarray(np.stack([gD, -gA, zero]), np.float32)
        want = self.sum_gradients(gC, g_comp)
        others = []
        for seed, contract in ((1, False), (2, True)):
            oracle.set_bwd_float_order(seed)
            oracle.set_bwd_contract(contract)
            try:
                others.append(self.sum_gradients(gC, g_comp))
            finally:
                oracle.set_bwd_float_order(0)
                oracle.set_bwd_contract(False)
        floor = {k: (max(util.rel_l2(f[k], want[k]) for f in others) if want[k].size else 0.0) for k in want}
        bound = {k: max(1e-4, NOISE_K * floor[k]) for k in want}
        return want, floor, bound


def compare_gradients(got, want, floor, bound, culled, what):
    """Every array of `got` (name -> numpy): finite, rel-L2 against `want` inside its bound, culled rows exactly zero.  Prints
    bound, floor and achieved value per array; -> {array: achieved}."""
    achieved = {}
    for k in util.GRAD_NAMES:
        g, w = got[k], want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.isfinite(g).all(), (what, k)
        if w.size == 0:
            continue
        rl = util.rel_l2(g, w)
        achieved[k] = rl
        print(f"[planes gradient] {what} {k}: bound {bound[k]:.1e}, float-order floor {floor[k]:.1e}, rel-L2 {rl:.2e}")
        if not np.any(w):   # (rel_l2 against an all-zero array is the norm itself: such an array has to BE zero)
            assert not np.any(g), (what, k, "gradient where the oracle has none", rl)
        assert rl <= bound[k], (what, k, rl, floor[k], bound[k])
        assert np.all(g[culled] == 0.0), (what, k, "a culled Gaussian has a gradient")
    return achieved
