"""TEST HELPER — GaussianAvatars' regularisers and density control restated in stock PyTorch over plain tensors and a
`torch.optim.Adam` whose state follows the rows (any dtype, any device): the reference of every rigged-density test.

reference:
  * regularisers — GaussianAvatarsLoss.accumulate_gradients, train/loss.py:367-379, on `exp(_scaling)` and `_xyz`
    (model/baseline/gaussianavatars.py:196-197); weights and thresholds of config/gaussianavatars.yaml:13-20
  * `binding_counter` — gaussianavatars.py:66-69
  * `_densify_and_prune` :278-295, `_clone_densify` :297-351, `_split_densify` :353-416, `_prune` :418-460,
    `_densification_postfix` :462-475, `_reset_opacity` :477-495; `build_rotation` tools/gs_utils/general_utils.py:78-99
The regularisers are pinned to a recorded run of `GaussianAvatarsLoss.accumulate_gradients` itself (the full loss, with the
D-SSIM image term) by tests/test_reference_runs_host.py (tests/golden/reference_image_terms.npz, case `ga`); the density-control
surgery stays builder-pinned (it needs a live optimiser and a rasterized frame).
`max_radii2D` is left out: `_densification_postfix` zeroes it in clone and in split immediately before the only test that
reads it (:289), so that test never fires."""
import torch

NAMES = ("_xyz", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling")   # train/optim.py:73-80
REFERENCE = dict(scale_weight=1.0, xyz_weight=0.01, threshold_scale=0.6, threshold_xyz=1.0)


def regularisers(scaling, xyz, threshold_scale=0.6, threshold_xyz=1.0):
    """(scale_loss, xyz_loss), unweighted, differentiable (train/loss.py:367-379)."""
    scale_loss = torch.relu(torch.exp(scaling) - threshold_scale).norm(dim=1).mean()
    xyz_loss = torch.relu(xyz.norm(dim=1) - threshold_xyz).mean()
    return scale_loss, xyz_loss


def regulariser_grads(scaling, xyz, scale_weight=1.0, xyz_weight=0.01, threshold_scale=0.6, threshold_xyz=1.0):
    """float64 autograd of `scale_weight * scale_loss + xyz_weight * xyz_loss`: (scale_loss, xyz_loss, d/d scaling,
    d/d xyz) as float64 tensors."""
    s = scaling.detach().double().clone().requires_grad_(True)
    x = xyz.detach().double().clone().requires_grad_(True)
    ls, lx = regularisers(s, x, threshold_scale, threshold_xyz)
    (scale_weight * ls + xyz_weight * lx).backward()
    return ls.detach(), lx.detach(), s.grad, x.grad


def gate_margins(scaling, xyz, threshold_scale=0.6, threshold_xyz=1.0):
    """(min relative distance of any exp(s) from threshold_scale, of any |xyz| from threshold_xyz), in float64."""
    e = torch.exp(scaling.double())
    n = xyz.double().norm(dim=1)
    return float(((e - threshold_scale).abs() / threshold_scale).min()), float(((n - threshold_xyz).abs() / threshold_xyz).min())


def draw_gate_inputs(P, generator, threshold_scale=0.6, threshold_xyz=1.0, dtype=torch.float32):
    """Seeded `_scaling` / `_xyz` [P,3] with components and rows on both sides of both gates, and some rows clipped to zero
    entirely.  Values that land within 3 % of a threshold are moved 6 % further (the caller CHECKS the margin it needs with
    gate_margins: this only makes the draw pass it)."""
    import math
    scaling = (torch.randn(P, 3, generator=generator, dtype=torch.float64) * 0.8 + math.log(threshold_scale) - 0.1)
    xyz = torch.randn(P, 3, generator=generator, dtype=torch.float64) * (0.7 * threshold_xyz)
    scaling, xyz = scaling.to(dtype), xyz.to(dtype)
    near = ((torch.exp(scaling.double()) - threshold_scale).abs() < 0.03 * threshold_scale)
    scaling = torch.where(near, scaling + math.log(1.06), scaling)
    near = ((xyz.double().norm(dim=1) - threshold_xyz).abs() < 0.03 * threshold_xyz)
    xyz = torch.where(near[:, None], xyz * 1.06, xyz)
    return scaling.contiguous(), xyz.contiguous()


def build_rotation(r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype, device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class RiggedRef:
    """The Gaussians of GaussianAvatars as six nn.Parameters in one Adam (one group each), `binding`, `binding_counter` and
    the densification statistics."""
    percent_dense = 0.01    # gaussianavatars.py:47

    def __init__(self, params: dict, binding, n_faces: int, lrs: dict = None):
        self.p = {n: torch.nn.Parameter(params[n].detach().clone()) for n in NAMES}
        lrs = lrs or {}
        self.opt = torch.optim.Adam([dict(params=[self.p[n]], lr=float(lrs.get(n, 1e-3)), name=n) for n in NAMES], lr=0.0)
        self.binding = binding.detach().clone().long()
        self.n_faces = int(n_faces)
        self.binding_counter = torch.bincount(self.binding, minlength=self.n_faces).to(torch.int32)     # :66-69
        P = self.binding.shape[0]
        dev = self.binding.device
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)

    @property
    def P(self):
        return int(self.binding.shape[0])

    def step(self, grads: dict):
        """One Adam step on the given gradients (creates the optimizer state)."""
        for n in NAMES:
            self.p[n].grad = grads[n].detach().clone().reshape(self.p[n].shape)
        self.opt.step()

    def moments(self, n):
        st = self.opt.state.get(self.p[n])
        return (None, None, None) if not st else (st["exp_avg"], st["exp_avg_sq"], st["step"])

    def set_moments(self, n, exp_avg, exp_avg_sq, step):
        """Gives parameter `n` the Adam state (exp_avg, exp_avg_sq, step count)."""
        p = self.p[n]
        self.opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": exp_avg.detach().clone().reshape(p.shape),
                             "exp_avg_sq": exp_avg_sq.detach().clone().reshape(p.shape)}

    # ---- optimizer surgery
    def _cat(self, ext: dict):
        for group in self.opt.param_groups:
            old, add = group["params"][0], ext[group["name"]]
            stored = self.opt.state.get(old, None)
            new = torch.nn.Parameter(torch.cat((old.detach(), add), dim=0))
            if stored is not None:
                stored["exp_avg"] = torch.cat((stored["exp_avg"], torch.zeros_like(add)), dim=0)        # :339-340
                stored["exp_avg_sq"] = torch.cat((stored["exp_avg_sq"], torch.zeros_like(add)), dim=0)
                del self.opt.state[old]
                self.opt.state[new] = stored
            group["params"][0] = new
            self.p[group["name"]] = new
        self._postfix()

    def _postfix(self):                                                                                 # :462-475
        dev = self.binding.device
        self.xyz_gradient_accum = torch.zeros((self.P, 1), device=dev)
        self.denom = torch.zeros((self.P, 1), device=dev)

    def _count(self, binding, sign):
        self.binding_counter.scatter_add_(0, binding, sign * torch.ones_like(binding, dtype=torch.int32))

    # ---- :297-351
    def clone_densify(self, grads, max_grad, extent):
        sel = torch.norm(grads, dim=-1) >= max_grad
        sel = sel & (torch.max(torch.exp(self.p["_scaling"].detach()), dim=1).values <= self.percent_dense * extent)
        ext = {n: self.p[n].detach()[sel] for n in NAMES}
        new_binding = self.binding[sel]
        self.binding = torch.cat([self.binding, new_binding])
        self._count(new_binding, 1)
        self._cat(ext)
        return int(sel.sum())

    # ---- :353-416
    def split_densify(self, grads, max_grad, extent, generator=None, N=2):
        P = self.P
        dev = self.binding.device
        padded = torch.zeros(P, device=dev)
        padded[:grads.shape[0]] = grads.squeeze(-1)
        scaling, rotation, xyz = (self.p[n].detach() for n in ("_scaling", "_rotation", "_xyz"))
        sel = (padded >= max_grad) & (torch.max(torch.exp(scaling), dim=1).values > self.percent_dense * extent)
        stds = torch.exp(scaling)[sel].repeat(N, 1)
        means = torch.zeros((stds.size(0), 3), device=dev)
        samples = torch.normal(mean=means, std=stds, generator=generator)
        rots = build_rotation(rotation[sel]).repeat(N, 1, 1)
        ext = {"_xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + xyz[sel].repeat(N, 1),
               "_scaling": torch.log(torch.exp(scaling[sel]).repeat(N, 1) / (0.8 * N)),
               "_rotation": rotation[sel].repeat(N, 1),
               "_features_dc": self.p["_features_dc"].detach()[sel].repeat(N, 1, 1),
               "_features_rest": self.p["_features_rest"].detach()[sel].repeat(N, 1, 1),
               "_opacity": self.p["_opacity"].detach()[sel].repeat(N, 1)}
        new_binding = self.binding[sel].repeat(N)
        self.binding = torch.cat((self.binding, new_binding))
        self._count(new_binding, 1)
        self._cat(ext)
        n = int(sel.sum())
        self.prune(torch.cat((sel, torch.zeros(N * n, device=dev, dtype=torch.bool))))
        return n

    # ---- :418-460
    def prune(self, mask):
        mask = mask.clone()
        binding_to_prune = self.binding[mask]
        counter_prune = torch.zeros_like(self.binding_counter)
        counter_prune.scatter_add_(0, binding_to_prune, torch.ones_like(binding_to_prune, dtype=torch.int32))
        mask_redundant = (self.binding_counter - counter_prune) > 0
        mask[mask.clone()] = mask_redundant[binding_to_prune]
        valid = ~mask
        for group in self.opt.param_groups:
            old = group["params"][0]
            stored = self.opt.state.get(old, None)
            new = torch.nn.Parameter(old.detach()[valid])
            if stored is not None:
                stored["exp_avg"] = stored["exp_avg"][valid]
                stored["exp_avg_sq"] = stored["exp_avg_sq"][valid]
                del self.opt.state[old]
                self.opt.state[new] = stored
            group["params"][0] = new
            self.p[group["name"]] = new
        self.xyz_gradient_accum = self.xyz_gradient_accum[valid]
        self.denom = self.denom[valid]
        self._count(self.binding[mask], -1)
        self.binding = self.binding[valid]
        return int(mask.sum())

    # ---- :278-295
    def densify_and_prune(self, max_grad=1e-4, min_opacity=0.005, extent=2.0, max_screen_size=None, generator=None):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        n_clone = self.clone_densify(grads, max_grad, extent)
        n_split = self.split_densify(grads, max_grad, extent, generator)
        mask = (torch.sigmoid(self.p["_opacity"].detach()) < min_opacity).squeeze(-1)
        if max_screen_size:
            mask = mask | (torch.exp(self.p["_scaling"].detach()).max(dim=1).values > 0.1 * extent)
        return n_clone, n_split, self.prune(mask)

    # ---- :477-495
    def reset_opacity(self):
        old = self.p["_opacity"]
        new_val = torch.min(torch.sigmoid(old.detach()), torch.ones_like(old) * 0.01)
        new_val = torch.log(new_val / (1 - new_val))                                       # inverse_sigmoid
        for group in self.opt.param_groups:
            if group["name"] == "_opacity":
                stored = self.opt.state.get(old, None)
                new = torch.nn.Parameter(new_val)
                if stored is not None:
                    stored["exp_avg"] = torch.zeros_like(new_val)
                    stored["exp_avg_sq"] = torch.zeros_like(new_val)
                    del self.opt.state[old]
                    self.opt.state[new] = stored
                group["params"][0] = new
                self.p["_opacity"] = new
