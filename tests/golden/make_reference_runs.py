"""Generate tests/golden/reference_*.npz: runs of the reference's OWN Python for the avatar losses, the point skinning, the
deformation MLP, the perceptual term and FLAME's posing with FateAvatar's deltas, recorded as plain data.

Runs ONLY in the build container (needs /root/reference); the fixtures it writes hold arrays, scalars and a `notes` string and
are committed.  No test imports this file.  Run as

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_reference_runs.py            (writes the fixtures)
    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_reference_runs.py --check    (compares a fresh run with the committed ones)

What is called, unmodified and on the CPU, in float32 and in float64 (float64 inputs; torch's default dtype stays float32
except where `both(..., default64=True)` says why not):
  tools/loss_utils/dssim.py           d_ssim
  train/loss.py                       SplattingAvatarLoss / FlashAvatarLoss / GaussianAvatarsLoss / MonoGaussianAvatarLoss
                                      .accumulate_gradients, FateAvatarLoss.get_laplacian_smoothing_loss / .accumulate_gradients
  flame/FLAME.py over flame/lbs.py    FLAME.forward_pts (inverse_pts, forward_pts)
  flame/lbs.py                        lbs, with the arguments FLAME.forward_with_delta_blendshape hands it
  model/baseline/flashavatar.py       Embedder, MLP, FlashAvatar.quatProduct_batch
  tools/loss_utils/vgg_feature.py     VGGPerceptualLoss (constructor and forward)
None of their text is in this file.  The work-arounds, all of them:
  * stand-in modules for what is not installed (pytorch3d.*, lpips, torchvision, plyfile, igl, simple_knn,
    diff_gaussian_rasterization, simple_phongsurf, matplotlib, PIL) through a meta-path finder APPENDED to sys.meta_path: a
    module that really is installed wins.  A stand-in module hands out one inert placeholder class for every name; nothing that
    computes is replaced — but for `torchvision.models.vgg16` and `VGG16_Weights`, which are made to work (below, at their
    definition: a narrow VGG-16 in torchvision's layout with seeded weights; the layout is builder-pinned).
    (FateAvatarLoss.accumulate_gradients constructs a pytorch3d `Meshes` it never reads once `laplacian_matrix` is set: that
    object is the placeholder.)
  * objects made with `__new__` + `nn.Module.__init__` and only the attributes the called method reads (the constructors
    build LPIPS / VGG networks or read the FLAME pickle);
  * `Tensor.cuda` returns the tensor itself while MonoGaussianAvatarLoss.get_gt_blendshape runs with a ghost bone (its one
    `.cuda()` call on the padded weight table); noted in the fixture's `notes`.
The Laplacian MATRIX is not the reference's: pytorch3d is absent, so `laplacian_matrix` is preset to
tests/mesh_terms_ref.laplacian_dense and the matrix rule itself stays pinned by the hand-written cases of
tests/test_mesh_terms_host.py.  What is recorded is what the reference does WITH the matrix.

Layout.  Every case has a name; its keys are
  <case>_in_<name>      an input, float32 (indices int32 / int64); both runs read these values
  <case>_param_<name>   a field of the reference's `Params` dataclass (or of config/fateavatar.yaml) the run used
  <case>_<output>       the reference's float64 result on those inputs: the truth
  <case>_<output>_e32   rel-L2 (scalars: relative difference) of the reference's own float32 run against that, a scalar
  <case>_margin...      how far the inputs keep from a gate (asserted here, so that no test leaves an element out)
An array that would carry a file over 1 MB is stored rounded to float32 and listed in `notes` (the MLP's weight gradients).
A group of cases that does not fit one file is split into reference_<group>.npz, reference_<group>_2.npz, ...;
tests/reference_runs.py loads them all into one dictionary.
"""
import copy
import dataclasses
import glob
import importlib.abc
import importlib.machinery
import math
import os
import sys
import types

import numpy as np
import torch
import yaml

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
FILE_BYTES = 950_000          # raw array bytes per file: the compressed file stays under 1 MB (asserted)
sys.dont_write_bytecode = True

STAND_INS = ("pytorch3d", "lpips", "torchvision", "plyfile", "igl", "simple_knn", "diff_gaussian_rasterization",
             "simple_phongsurf", "matplotlib", "PIL")


class Placeholder:
    """What a stand-in module hands out for any name: it can be constructed and does nothing."""

    def __init__(self, *args, **kwargs):
        pass


class StandIn(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return Placeholder


class StandInFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in STAND_INS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return StandIn(spec.name)

    def exec_module(self, module):
        pass


# the reference first (its `tools`, `train`, `flame`, `model` packages), with nothing of this repository on the path yet: the
# repository's own `simple_knn` / `diff_gaussian_rasterization` drop-ins must not be what the reference's imports find
sys.path.insert(0, REF)
sys.meta_path.append(StandInFinder())


# torchvision is not installed, and VGGPerceptualLoss's constructor asks it for a pretrained VGG-16 four times.  Two names of the
# stand-in are therefore made to WORK before the reference's module is imported: `models.vgg16(weights=...)` returns an object whose
# `.features` is an nn.Sequential in torchvision's configuration-D layout (conv, ReLU(inplace), conv, ReLU, MaxPool2d(2, 2), ...
# through index 22, the last the reference slices), every width 64 (tests/vgg_ref.NARROW), with tests/vgg_ref.he_weights'
# weights — the same on every call — and `models.VGG16_Weights.DEFAULT` exists.  The LAYOUT is this file's reading of
# torchvision, not torchvision's own code: it stays builder-pinned.
VGG_SEED = 29


class NarrowVgg16Weights:
    DEFAULT = "DEFAULT"


def narrow_vgg16(weights=None):
    from tests import vgg_ref
    assert weights is NarrowVgg16Weights.DEFAULT
    W, B = vgg_ref.he_weights(vgg_ref.NARROW, VGG_SEED)
    mods = []
    for (ci, co, pool, tap), w, b in zip(vgg_ref.NARROW, W, B):
        if pool:
            mods.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
        conv = torch.nn.Conv2d(ci, co, kernel_size=3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        mods += [conv, torch.nn.ReLU(inplace=True)]
    holder = torch.nn.Module()
    holder.features = torch.nn.Sequential(*mods)
    return holder


import torchvision.models  # noqa: E402
assert isinstance(torchvision.models, StandIn), "torchvision is installed: record with its own vgg16 layout and say so in DESIGN.md"
torchvision.models.vgg16, torchvision.models.VGG16_Weights = narrow_vgg16, NarrowVgg16Weights

from flame.FLAME import FLAME  # noqa: E402
from flame.lbs import lbs as ref_lbs  # noqa: E402
from model.baseline.flashavatar import MLP, Embedder, FlashAvatar  # noqa: E402
from tools.loss_utils.dssim import d_ssim  # noqa: E402
from tools.loss_utils.vgg_feature import VGGPerceptualLoss  # noqa: E402
from train import loss as ref_loss  # noqa: E402

sys.path.insert(1, ROOT)
from tests import flame_ref, image_loss_ref, mesh_terms_ref, mono_ref, rigged_density_ref, splatting_loss_ref, vgg_ref  # noqa: E402
from tests.test_gpu_mlp import SEED_MARGIN, _keeps_clear_of_zero  # noqa: E402
from tests.test_gpu_mono import _row_metric  # noqa: E402
from tests.test_gpu_mono_pose import _element_metric  # noqa: E402

NOTES = []


# ---------------------------------------------------------------- helpers
def bare(cls, **attrs):
    obj = cls.__new__(cls)
    torch.nn.Module.__init__(obj)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def both(fn, default64=False):
    """fn(dtype) -> dict of tensors; (its float32 results, its float64 results).  `default64`: torch's default dtype is float64
    during the float64 run, for the one method that creates a tensor it computes with in the default dtype (the ghost bone's
    weight table).  Everywhere else the default stays float32: d_ssim builds its window with `torch.Tensor(...)`, and under
    a float64 default that would be ANOTHER window than the one every real run uses."""
    r32 = fn(torch.float32)
    if default64:
        torch.set_default_dtype(torch.float64)
    try:
        r64 = fn(torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
    for k in r64:
        assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64, (k, r32[k].dtype, r64[k].dtype)
    return r32, r64


def rel(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).norm())


def record(out, case, inputs, r32, r64, params=None, as_float32=()):
    for k, v in inputs.items():
        v = v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        assert v.dtype in (np.float32, np.int32, np.int64), (case, k, v.dtype)
        out[f"{case}_in_{k}"] = v
    for k, v in (params or {}).items():
        out[f"{case}_param_{k}"] = np.float64(v)
    for k in r64:
        a = r64[k].detach().numpy()
        out[f"{case}_{k}"] = a.astype(np.float32) if k in as_float32 else a
        out[f"{case}_{k}_e32"] = np.float64(rel(r32[k], r64[k]))
        if k in as_float32:
            NOTES.append(f"{case}_{k} is the float64 result rounded to float32 (the array would carry its file over 1 MB)")
    shown = ", ".join(f"{k} {float(out[f'{case}_{k}_e32']):.1e}" for k in r64)
    print(f"{case}: e32 {shown}")


def number_fields(params):
    return {k: v for k, v in dataclasses.asdict(params).items() if isinstance(v, (int, float)) and not isinstance(v, bool)}


def detached(d):
    return {k: v.detach() for k, v in d.items()}


# ---------------------------------------------------------------- the image terms
def case_dssim(out, case, shape):
    x, y = image_loss_ref.make_inputs(shape, "near")

    def run(dt):
        xx = leaf(x[None], dt)
        loss = d_ssim(xx, y[None].to(dt))
        (g,) = torch.autograd.grad(loss, xx)
        return dict(loss=loss.detach(), d_img=g[0])

    record(out, case, dict(img=x, gt=y), *both(run))


def case_splatting(out, case="splat"):
    shape, P = (3, 37, 53), 1000
    img, gt = image_loss_ref.make_inputs(shape, "noise", seed=1)
    params = ref_loss.SplattingAvatarLoss.Params(lpips_weight=0.0)
    gen = torch.Generator().manual_seed(41)
    s = splatting_loss_ref.draw_scaling(P, gen, params.scale_threshold, params.max_scaling)
    assert not bool(splatting_loss_ref.undecided_rows(s, params.scale_threshold, params.max_scaling).any())
    scale = torch.exp(s.double())
    smax, smin = scale.max(1).values, scale.min(1).values
    margin = float(torch.minimum((smax / params.max_scaling - 1).abs(), (smax / smin / params.scale_threshold - 1).abs()).min())
    assert margin > 1e-4
    out[f"{case}_margin"] = np.float64(margin)

    def run(dt):
        L = bare(ref_loss.SplattingAvatarLoss, params=params, l1_loss=torch.nn.L1Loss(reduction="mean"),
                 l2_loss=torch.nn.MSELoss(reduction="mean"))
        x, raw = leaf(img[None], dt), leaf(s, dt)
        o = L.accumulate_gradients({"rgb_image": x, "scale": torch.exp(raw)}, {"rgb": gt[None].to(dt)})
        assert sorted(o) == ["loss", "mse_loss", "rgb_loss", "scale_loss"]
        gx, gs = torch.autograd.grad(o["loss"], (x, raw))
        return dict(detached(o), d_img=gx[0], d_scaling=gs)

    r32, r64 = both(run)
    assert float(r64["scale_loss"]) > 0
    record(out, case, dict(img=img, gt=gt, scaling=s), r32, r64, number_fields(params))


def case_flash(out, case, masked):
    shape = (3, 37, 53)
    img, gt = image_loss_ref.make_inputs(shape, "noise", seed=2)
    gen = torch.Generator().manual_seed(43)
    mask = torch.rand((1,) + shape[1:], generator=gen)
    mask.view(-1)[0::7], mask.view(-1)[3::11] = 1.0, 0.0
    params = ref_loss.FlashAvatarLoss.Params(lpips_weight=0.0)

    def run(dt):
        L = bare(ref_loss.FlashAvatarLoss, params=params)
        x = leaf(img[None], dt)
        o = L.accumulate_gradients({"rgb_image": x}, {"rgb": gt[None].to(dt), "mouth_mask": mask[None].to(dt) if masked else None})
        assert sorted(o) == ["huber_loss", "loss"]
        (g,) = torch.autograd.grad(o["loss"], x)
        return dict(loss=o["loss"].detach(), d_img=g[0])

    inputs = dict(img=img, gt=gt)
    if masked:
        inputs["mask"] = mask
    record(out, case, inputs, *both(run), number_fields(params))


def case_gaussianavatars(out, case="ga"):
    P = 1000
    img, gt = image_loss_ref.make_inputs((3, 33, 47), "near")          # the D-SSIM image of the first case
    params = ref_loss.GaussianAvatarsLoss.Params()
    s, xyz = rigged_density_ref.draw_gate_inputs(P, torch.Generator().manual_seed(47), params.threshold_scale, params.threshold_xyz)
    ms, mx = rigged_density_ref.gate_margins(s, xyz, params.threshold_scale, params.threshold_xyz)
    assert ms >= 0.01 and mx >= 0.01, (ms, mx)
    out[f"{case}_margin_scale"], out[f"{case}_margin_xyz"] = np.float64(ms), np.float64(mx)

    def run(dt):
        L = bare(ref_loss.GaussianAvatarsLoss, params=params, l1_loss=torch.nn.L1Loss(reduction="mean"))
        x, raw, p = leaf(img[None], dt), leaf(s, dt), leaf(xyz, dt)
        o = L.accumulate_gradients({"rgb_image": x, "scale": torch.exp(raw), "xyz": p}, {"rgb": gt[None].to(dt)})
        assert sorted(o) == ["dssim_loss", "loss", "rgb_loss", "scale_loss", "xyz_loss"]
        gx, gs, gp = torch.autograd.grad(o["loss"], (x, raw, p))
        return dict(detached(o), d_img=gx[0], d_scaling=gs, d_xyz=gp)

    r32, r64 = both(run)
    assert float(r64["scale_loss"]) > 0 and float(r64["xyz_loss"]) > 0
    record(out, case, dict(img=img, gt=gt, scaling=s, xyz=xyz), r32, r64, number_fields(params))


# ---------------------------------------------------------------- FateAvatar's mesh terms
def case_fate(out, case="fate"):
    V, seed, flame_weight = 65, 101, 0.3
    vo, faces = mesh_terms_ref.random_mesh(V, seed)
    v = mesh_terms_ref.displaced(vo, seed)
    vo, v = torch.from_numpy(vo), torch.from_numpy(v)
    img, gt = image_loss_ref.make_inputs((3, 7, 5), "noise", seed=3)
    with open(os.path.join(REF, "config", "fateavatar.yaml")) as f:
        w = yaml.safe_load(f)["loss"]["weight"]
    P = ref_loss.FateAvatarLoss.Params
    # config/fateavatar.yaml's weights of the terms that run without a network: rgb, laplacian, normal, flame
    configured = P(rgb_weight=w["rgb_loss"], laplacian_weight=w["laplacian_loss"], normal_weight=w["normal_loss"],
                   flame_weight=w["flame_loss"])
    with_flame = P(rgb_weight=w["rgb_loss"], flame_weight=flame_weight)
    assert configured.normal_weight == 0

    def make(params, dt):
        return bare(ref_loss.FateAvatarLoss, params=params, l1_loss=torch.nn.L1Loss(reduction="mean"),
                    l2_loss=torch.nn.MSELoss(reduction="mean"), laplacian_matrix=mesh_terms_ref.laplacian_dense(faces, V, dt))

    def run(dt):
        res = {}
        vv = leaf(v[None], dt)
        lap = make(configured, dt).get_laplacian_smoothing_loss(vo[None].to(dt), vv)
        res["laplacian_loss"], res["laplacian_d_verts"] = lap.detach(), torch.autograd.grad(lap, vv)[0][0]
        for name, params, keys in (("configured", configured, ["laplacian_loss", "loss", "rgb_loss"]),
                                   ("flame", with_flame, ["flame_loss", "loss", "rgb_loss"])):
            vv = leaf(v[None], dt)
            o = make(params, dt).accumulate_gradients({"rgb_image": img[None].to(dt), "verts": vv, "verts_orig": vo[None].to(dt),
                                                       "faces": torch.from_numpy(faces)}, {"rgb": gt[None].to(dt)})
            assert sorted(o) == keys, sorted(o)
            # (this class's out['rgb_loss'] IS out['loss'], one tensor added to in place: it is not recorded a second time)
            assert o["rgb_loss"] is o["loss"]
            for k in keys[:2]:
                res[f"{name}_{k}"] = o[k].detach()
            res[f"{name}_d_verts"] = torch.autograd.grad(o["loss"], vv)[0][0]
        return res

    record(out, case, dict(verts_orig=vo, verts=v, faces=faces.astype(np.int64), img=img, gt=gt), *both(run),
           dict(rgb_weight=configured.rgb_weight, laplacian_weight=configured.laplacian_weight,
                configured_flame_weight=configured.flame_weight, flame_weight=flame_weight))
    NOTES.append("fate: laplacian_matrix is tests/mesh_terms_ref.laplacian_dense, not pytorch3d's (absent): the matrix rule stays "
                 "hand-pinned; `configured` uses config/fateavatar.yaml's rgb / laplacian / normal / flame weights")


# ---------------------------------------------------------------- MonoGaussianAvatar's blendshape terms
def case_mono_terms(out, case, N, V, E, J, with_var, seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    ghost = J == 6
    assert J in (5, 6)
    pred = dict(lbs_weights=torch.softmax(rn(N, J), 1), posedirs=0.01 * rn(N, 36, 3), shapedirs=0.01 * rn(N, 3, E))
    tables = dict(flame_lbs_weights=torch.softmax(rn(V, 5), 1), flame_posedirs=0.01 * rn(36, 3 * V), flame_shapedirs=0.01 * rn(V, 3, E))
    index = torch.randint(0, V, (N,), generator=gen)
    index[0], index[1] = 0, V - 1
    var = (0.5 + torch.rand(E, generator=gen)) if with_var else None
    image = torch.zeros(1, 3, 2, 2)

    def run(dt):
        params = ref_loss.MonoGaussianAvatarLoss.Params(rgb_weight=0.0, vgg_weight=0.0, dssim_weight=0.0,
                                                        var_expression=None if var is None else var.to(dt), GT_lbs_milestones=[])
        L = bare(ref_loss.MonoGaussianAvatarLoss, params=params, l1_loss=torch.nn.L1Loss(reduction="mean"),
                 l2_loss=torch.nn.MSELoss(reduction="mean"))
        if ghost:
            inner = L.get_gt_blendshape

            def on_the_cpu(*a, **k):
                cuda = torch.Tensor.cuda
                torch.Tensor.cuda = lambda self, *aa, **kk: self
                try:
                    return inner(*a, **k)
                finally:
                    torch.Tensor.cuda = cuda
            L.get_gt_blendshape = on_the_cpu
        leaves = {k: leaf(t, dt) for k, t in pred.items()}
        o = L.accumulate_gradients(dict(leaves, rgb_image=image.to(dt), index_batch=index, **{k: t.to(dt) for k, t in tables.items()}),
                                   {"rgb": image.to(dt)}, cur_epoch=0)
        assert sorted(o) == ["lbs_loss", "loss", "posedirs_loss", "rgb_loss", "shapedirs_loss"] and float(o["rgb_loss"]) == 0
        grads = torch.autograd.grad(o["loss"], list(leaves.values()))
        res = {k: o[k].detach() for k in ("lbs_loss", "posedirs_loss", "shapedirs_loss", "loss")}
        res.update({f"d_{k}": g for k, g in zip(leaves, grads)})
        return res

    inputs = dict(pred, index=index, **tables)
    if var is not None:
        inputs["var_expression"] = var
    record(out, case, inputs, *both(run, default64=ghost), dict(lbs_weight=ref_loss.MonoGaussianAvatarLoss.Params().lbs_weight))
    if ghost:
        NOTES.append(f"{case}: Tensor.cuda returned the tensor itself while get_gt_blendshape ran (its ghost-bone `.cuda()` call)")


# ---------------------------------------------------------------- MonoGaussianAvatar's point skinning
def skinning_run(N, E, J):
    p, S, P, w, c, f, g = [t.float() if isinstance(t, torch.Tensor) else tuple(x.float() for x in t) for t in mono_ref.recipe(N, E, J)]

    def run(dt):
        fl = bare(FLAME, n_exp=E, canonical_exp=c[0].to(dt)[None], canonical_pose_feature=c[1].to(dt)[None],
                  canonical_transformations=c[2].to(dt)[None])
        leaves = [leaf(t, dt) for t in (p, S, P, w, f[0], f[1], f[2])]
        pts, sd, pd, lw, betas, feature, A = leaves
        xyz = fl.forward_pts(pts, betas[None].expand(N, -1), A[None].expand(N, -1, -1, -1), feature[None].expand(N, -1), sd, pd, lw,
                             dtype=dt)
        grads = torch.autograd.grad(xyz, leaves, g.to(dt))
        names = ("points", "shapedirs", "posedirs", "lbs_weights", "betas", "pose_feature", "transforms")
        return dict(xyz=xyz.detach(), **{f"d_{n}": t for n, t in zip(names, grads)})

    inputs = dict(points=p, shapedirs=S, posedirs=P, lbs_weights=w, canonical_betas=c[0], canonical_pose_feature=c[1],
                  canonical_transforms=c[2], betas=f[0], pose_feature=f[1], transforms=f[2], g=g)
    return inputs, both(run)


def case_skinning(out, case, N, E, J):
    inputs, (r32, r64) = skinning_run(N, E, J)
    record(out, case, inputs, r32, r64)
    # the yardsticks of tests/test_gpu_mono.py (ROW_FACTOR) and tests/test_gpu_mono_pose.py (ELEMENT_FACTOR): the worst row /
    # element of the REFERENCE's float32 run against its float64 run at N = 4 099 of the same recipe (a maximum over a few
    # rows is no yardstick, as those tests explain); only the scalars are stored
    _, (b32, b64) = skinning_run(4099, E, J)
    for n in ("points", "shapedirs", "posedirs", "lbs_weights"):
        out[f"{case}_d_{n}_row32"] = np.float64(_row_metric(b32[f"d_{n}"], b64[f"d_{n}"]).max())
    for n in ("betas", "pose_feature", "transforms"):
        out[f"{case}_d_{n}_element32"] = np.float64(_element_metric(b32[f"d_{n}"], b64[f"d_{n}"]).max())
    out[f"{case}_xyz_max32"] = np.float64((r32["xyz"].double() - r64["xyz"]).abs().max())


# ---------------------------------------------------------------- FlashAvatar's embedding, MLP and quaternion product
def case_mlp(out, case="mlp"):
    N, De, Dc, L = 257, 51, 59, 2
    rng = torch.get_rng_state()
    torch.manual_seed(17 + De + Dc + L)
    net = MLP(De + Dc, 10, 256, L)
    torch.set_rng_state(rng)
    embedder = Embedder(8)
    assert embedder.dim_embeded == De
    W = [fc.weight.detach() for fc in net.fcs] + [net.output_linear.weight.detach()]
    B = [fc.bias.detach() for fc in net.fcs] + [net.output_linear.bias.detach()]
    W64, B64 = [t.double() for t in W], [t.double() for t in B]
    for attempt in range(400):                     # the redraw rule of tests/test_gpu_mlp.py
        g = torch.Generator().manual_seed(1000 * De + 10 * Dc + L + 7 * N + 100003 * attempt)
        pts = torch.rand(N, 3, generator=g) * 0.4 - 0.2
        E = embedder(pts[None])[0].contiguous()
        cond = 0.5 * torch.randn(Dc, generator=g)
        d_out = torch.randn(N, 10, generator=g)
        if _keeps_clear_of_zero(W64, B64, E, cond):
            break
    else:
        raise AssertionError("no seed keeps the float64 pre-activations clear of zero")
    with torch.no_grad():
        h, margin = torch.cat([E.double(), cond.double().expand(N, Dc)], dim=1), math.inf
        for w, b in zip(W64[:-1], B64[:-1]):
            z = torch.nn.functional.linear(h, w, b)
            margin = min(margin, float(z.abs().min()) / float(z.pow(2).mean().sqrt()))
            h = torch.relu(z)
    assert margin >= SEED_MARGIN
    out[f"{case}_margin"] = np.float64(margin)

    def run_embed(dt):
        return dict(embed=Embedder(8)(pts.to(dt)[None])[0])

    def run(dt):
        n = copy.deepcopy(net).to(dt)
        c = leaf(cond[None], dt)                                    # [1,Dc], as `forward` has it
        fed = torch.cat([E.to(dt)[None], c.unsqueeze(1).repeat(1, N, 1)], dim=2)
        o = n(fed)
        o.backward(d_out.to(dt)[None])
        layers = list(n.fcs) + [n.output_linear]
        res = dict(out=o.detach()[0], d_cond=c.grad[0])
        res["d_weights"] = torch.cat([m.weight.grad.reshape(-1) for m in layers])
        res["d_bias"] = torch.cat([m.bias.grad.reshape(-1) for m in layers])
        return res

    record(out, "embed", dict(points=pts), *both(run_embed))
    inputs = dict(E=E, cond=cond, d_out=d_out)
    for i, (w, b) in enumerate(zip(W, B)):
        inputs[f"weight_{i}"], inputs[f"bias_{i}"] = w, b
    record(out, case, inputs, *both(run), as_float32=("d_weights",))
    NOTES.append(f"{case}: weights and inputs by the redraw rule of tests/test_gpu_mlp.py, attempt {attempt + 1}; d_weights / d_bias "
                 "are the layers' gradients flattened and concatenated, the output layer last")

    gen = torch.Generator().manual_seed(64)
    q1 = torch.nn.functional.normalize(torch.randn(64, 4, generator=gen), dim=1)
    q2 = torch.randn(64, 4, generator=gen)
    record(out, "quat", dict(q1=q1, q2=q2), *both(lambda dt: dict(product=FlashAvatar.quatProduct_batch(q1.to(dt), q2.to(dt)))))


# ---------------------------------------------------------------- FateAvatar's perceptual term
def case_vgg(out, case="vgg"):
    """VGGPerceptualLoss()(img[None], gt[None]) as it is — its own normalisation, its resize to 224^2, its four slices of the
    (narrow, stand-in) vgg16 — and its autograd gradient."""
    H, W = 37, 53
    img, gt = vgg_ref.images(H, W, seed=1000 * H + W)
    Wt, B = vgg_ref.he_weights(vgg_ref.NARROW, VGG_SEED)

    def run(dt):
        net = VGGPerceptualLoss().to(dt)
        assert len(net.blocks) == 4 and sum(len(b) for b in net.blocks) == 23 and net.mean.dtype == dt
        x = leaf(img[None], dt)
        loss = net(x, gt[None].to(dt))
        (g,) = torch.autograd.grad(loss, x)
        return dict(loss=loss.detach(), d_img=g[0])

    r32, r64 = both(run)
    inputs = dict(img=img, gt=gt)
    for i, (w, b) in enumerate(zip(Wt, B)):
        inputs[f"weight_{i}"], inputs[f"bias_{i}"] = w, b
    record(out, case, inputs, dict(loss=r32["loss"]), dict(loss=r64["loss"]))
    out[f"{case}_loss32"] = r32["loss"].numpy()
    out[f"{case}_d_img"] = r64["d_img"].numpy()
    NOTES.append(f"{case}: torchvision.models.vgg16 is this script's stand-in (configuration D's layout through features[22], every width "
                 f"64, tests/vgg_ref.he_weights(NARROW, {VGG_SEED})): the layout is builder-pinned, everything the reference does with it is "
                 f"recorded.  {case}_d_img is the float64 gradient; NO float32 gradient error is recorded or to be held: at 224^2 the "
                 f"reference's own float32 gradient is {rel(r32['d_img'], r64['d_img']):.1e} rel-L2 from its float64 one (ReLU masks, pool "
                 "argmaxes and tap signs that float32 rounding carries across their thresholds), which is no yardstick for a kernel — "
                 "the pinned backward of tests/vgg_ref.py at the device's own decisions is")


# ---------------------------------------------------------------- FLAME with FateAvatar's deltas
FLAME_SHAPE, FLAME_SEED = (65, 2, 5), 131


def flame_poses():
    """{case: (parents, pose [15] float32)}: joint trees other than FLAME's own, and the pose regimes a track has — exact zeros,
    rotations where float32's cos rounds to 1, rotations near pi and near 2 pi."""
    g = torch.Generator().manual_seed(FLAME_SEED + 1)
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)  # noqa: E731
    axes = torch.nn.functional.normalize(rn(5, 3), dim=1)
    rest = 0.3 * rn(5, 3)
    rest[[1, 3, 4]] = 0.0
    large = 3.1 * axes
    large[2] = 6.2 * axes[2]
    flame = (-1, 0, 1, 1, 1)
    cases = dict(flame_chain=((-1, 0, 1, 2, 3), 0.3 * rn(5, 3)), flame_star=((-1, 0, 0, 0, 0), 0.3 * rn(5, 3)),
                 flame_tree_small=((-1, 0, 0, 1, 2), 2e-4 * axes), flame_zero=(flame, torch.zeros(5, 3, dtype=torch.float64)),
                 flame_rest=(flame, rest), flame_large=(flame, large))
    return {k: (p, r.reshape(15).float()) for k, (p, r) in cases.items()}


def case_flame(out, case, m, parents, pose, store_tables):
    """lbs() as FLAME.forward_with_delta_blendshape calls it — betas = (zeros [1, NS], expression), the deltas added to the
    tables — on the tables of tests/flame_ref.random_model, and the gradients of sum(verts * g)."""
    NS = m["n_shape"]
    par = torch.tensor(parents, dtype=torch.long)

    def run(dt):
        c = lambda k: m[k].to(dt)  # noqa: E731
        dS, dP, dV, e, p = (leaf(t, dt) for t in (m["delta_shapedirs"], m["delta_posedirs"], m["delta_vertex"], m["expression"], pose))
        betas = torch.cat([torch.zeros(1, NS, dtype=dt), e[None]], dim=1)
        verts, phi, A = ref_lbs(betas, p[None], (c("v_template") + dV)[None], c("shapedirs") + dS, c("posedirs") + dP,
                                c("J_regressor"), par, c("lbs_weights"), dtype=dt)
        grads = torch.autograd.grad((verts[0] * c("g")).sum(), (dS, dP, dV, e, p))
        # the shape columns meet exact zeros: their gradient is exactly zero, and only that is recorded of them
        assert int(grads[0][:, :, :NS].count_nonzero()) == 0
        return dict(verts=verts[0].detach(), pose_feature=phi[0].detach(), A=A[0].detach(), d_delta_exp=grads[0][:, :, NS:].contiguous(),
                    d_delta_posedirs=grads[1], d_delta_vertex=grads[2], d_expression=grads[3], d_pose=grads[4])

    inputs = dict(parents=np.asarray(parents, dtype=np.int64), pose=pose)
    if store_tables:
        inputs.update({k: m[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "delta_shapedirs",
                                          "delta_posedirs", "delta_vertex", "expression", "g")})
    record(out, case, inputs, *both(run), dict(n_shape=NS, n_exp=m["n_exp"]))


# ---------------------------------------------------------------- files
def split(group, arrays):
    """[(file name, dict)]: the arrays in order, a new file whenever the next one would carry the file over FILE_BYTES."""
    files, cur, size = [], {}, 0
    for k, v in arrays.items():
        n = np.asarray(v).nbytes
        if cur and size + n > FILE_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    files.append(cur)
    return [(f"reference_{group}.npz" if i == 0 else f"reference_{group}_{i + 1}.npz", d) for i, d in enumerate(files)]


def main(check):
    groups = {}

    def group(name):
        NOTES.clear()
        return {}

    o = group("image_terms")
    case_dssim(o, "dssim_3x33x47", (3, 33, 47))
    case_dssim(o, "dssim_1x7x5", (1, 7, 5))
    case_splatting(o)
    case_flash(o, "huber_plain", masked=False)
    case_flash(o, "huber_mouth", masked=True)
    case_gaussianavatars(o)
    case_fate(o)
    groups["image_terms"] = (o, list(NOTES))
    o = group("mono_terms")
    case_mono_terms(o, "lbs_ghost", 300, 77, 50, 6, with_var=False, seed=71)
    case_mono_terms(o, "lbs_var_ghost", 300, 77, 50, 6, with_var=True, seed=71)
    case_mono_terms(o, "lbs_e7_j5", 300, 77, 7, 5, with_var=False, seed=73)
    # (the variance case reads the inputs of the case before it: they are stored once)
    for k in [k for k in o if k.startswith("lbs_var_ghost_in_") and k != "lbs_var_ghost_in_var_expression"]:
        assert np.array_equal(o[k], o[k.replace("lbs_var_ghost_in_", "lbs_ghost_in_")])
        del o[k]
    NOTES.append("lbs_var_ghost reads lbs_ghost's inputs (`lbs_ghost_in_*`) and its own `lbs_var_ghost_in_var_expression`")
    groups["mono_terms"] = (o, list(NOTES))
    o = group("skinning")
    case_skinning(o, "skin_65_50_6", 65, 50, 6)
    case_skinning(o, "skin_257_7_5", 257, 7, 5)
    groups["skinning"] = (o, list(NOTES))
    o = group("mlp")
    case_mlp(o)
    groups["mlp"] = (o, list(NOTES))
    o = group("vgg")
    case_vgg(o)
    groups["vgg"] = (o, list(NOTES))
    o = group("flame")
    m = flame_ref.random_model(*FLAME_SHAPE, seed=FLAME_SEED)
    for i, (name, (parents, pose)) in enumerate(flame_poses().items()):
        case_flame(o, name, m, parents, pose, store_tables=i == 0)
    NOTES.append("flame_*: every case reads flame_chain's tables, deltas, expression and g (`flame_chain_in_*`) and its own "
                 "`_in_parents` and `_in_pose`; d_delta_exp is the expression columns of the gradient of delta_shapedirs, whose shape "
                 "columns were asserted exactly zero; flame_zero's pose_feature and d_delta_posedirs are exactly zero (their e32 is "
                 "the plain norm of the float32 run)")
    groups["flame"] = (o, list(NOTES))

    wanted = set()
    for name, (arrays, notes) in groups.items():
        for fname, part in split(name, arrays):
            path = os.path.join(OUT, fname)
            wanted.add(path)
            if check:
                with np.load(path) as have:
                    assert sorted(have.files) == sorted(list(part) + ["notes"]), fname
                    worst = max(rel(torch.from_numpy(np.atleast_1d(have[k]).astype(np.float64)),
                                    torch.from_numpy(np.atleast_1d(np.asarray(part[k])).astype(np.float64))) for k in part)
                    same = all(np.array_equal(have[k], part[k]) for k in part)
                print(f"{fname}: {'identical arrays' if same else f'DIFFERS, worst rel-L2 {worst:.3e}'}")
                assert same, fname
                continue
            np.savez_compressed(path, notes=np.array("\n".join(notes)), **part)
            size = os.path.getsize(path)
            print("wrote", path, size, "bytes")
            assert size <= 1_000_000, (path, size)
    stale = set(glob.glob(os.path.join(OUT, "reference_*.npz"))) - wanted
    assert not stale, f"files of an earlier layout: {sorted(stale)}"


if __name__ == "__main__":
    main(check="--check" in sys.argv[1:])
