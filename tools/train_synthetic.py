#!/usr/bin/env python
"""the per-frame optimisation loop on a synthetic multi-view sequence.

    python tools/train_synthetic.py [--P 100000 --res 512 --views 8 --steps 300]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 tools/train_synthetic.py ...

Targets are renders of a hidden "ground-truth" Gaussian set on the head template from `--views` cameras (the FLAME
weights are absent: declared stand-in for the INSTA sequence); the trained set starts from perturbed appearance and
opacity.  Prints one JSON line: optimisation steps/s (render + L1 + backward + densification statistics + Adam, one
frame per rank per step, one flat-gradient all-reduce when N > 1) and the loss before / after.

    python tools/train_synthetic.py --fateavatar --train-mesh [--mesh-terms LAP FLAME --mesh-lr 1e-4]
FateAvatar's step with the OTHER half of the model: the targets come from a template displaced by a seeded smooth bump, a
torch `delta_vertex` leaf [V,3] is added to the template in front of the sequence's rigid and jaw motion and trained by
torch.optim.Adam through `step.d_verts` (the step's dLoss/dposed_verts, the reference's mesh terms already in it; `verts_orig`
is the undisplaced posed mesh).  Prints steps/s, the image loss, both mesh terms and |delta - bump| at start and end.
--vertex-grad alone: the plain loop with the vertex gradient switched on (what that option costs).
    python tools/train_synthetic.py --fateavatar --fused-flame [--flame-shape 100 --flame-exp 50 --mesh-terms LAP FLAME]
    python tools/train_synthetic.py --fateavatar --torch-flame [...]
FateAvatar's WHOLE iteration: a synthetic FLAME over the (centred) template (fateavatar_amd/flame.py: `synthetic_flame`), per
frame an expression and a pose, targets from the mesh with a seeded smooth bump as the true `delta_vertex`.  --fused-flame:
`AvatarStep(flame=FlameMesh, mesh_terms=...)` — FLAME forward (both meshes), frame, mesh terms, FLAME backward and both Adams in
ONE replayed graph.  --torch-flame: the A/B, the same loop with FLAME as the stock-PyTorch restatement (tests/flame_ref.py: needs
the checkout's tests/ next to tools/) run twice in front of the step, `posed.backward(step.d_verts)` and torch.optim.Adam over the
reference's three groups (delta_shapedirs at its full [V,3,L]).  Prints steps/s, the image loss, both mesh terms and
|delta_vertex - bump| at start and end.
    python tools/train_synthetic.py --fateavatar --perceptual [--fused-flame] [--vgg-weights FILE] [--perceptual-size 224]
    python tools/train_synthetic.py --fateavatar --torch-perceptual [...]
FateAvatar's VGG perceptual term at weight 0.1 in the step: `AvatarStep(perceptual=Perceptual(VggFeatures.vgg16()))` — one call
behind the L1 launch adds its gradient to the L1 gradient (csrc/fr_vgg.hip).  Seeded He-normal weights unless --vgg-weights names
a torch-saved state dict in torchvision's naming.  --torch-perceptual: the A/B, the same term at the same place through
F.conv2d and autograd.  The report gains `perceptual_loss` (the sum of the tap terms, then the terms).
    python tools/train_synthetic.py --fateavatar --scale-term [--fused-flame --perceptual | --train-mesh | --views-per-step K]
FateAvatar's scale-ratio term at weight 0.1, threshold 9.0 in the step: `AvatarStep(scale_term=REFERENCE_SCALE_TERM)` — one launch
behind the backward adds its gradient to `_scaling`'s in front of Adam (csrc/fr_optim.hip, `k_scale_ratio_term`); with
--fused-flame --perceptual the reference's whole objective.  The report gains `reg_loss` (scale_loss, rows over the threshold).
    python tools/train_synthetic.py --fateavatar --track-camera [--track-offset 0.005]
FateAvatar's step with the reference's camera tracking next to it (train/base.py:123,142: one translation per frame in an
embedding, at `tracking_lr`): every frame's camera translation is a torch leaf that starts --track-offset metres (RMS per axis)
from the truth; each step the frame's camera is built from it as `model.PoseCamera` builds it, rendered by
AvatarStep(camera_grad=True), and `step.d_view / d_proj / d_campos` are chained back through that construction into
torch.optim.Adam(lr=5e-4).  Prints steps/s, the image loss and the RMS translation error before and after.

    python tools/train_synthetic.py --bake [--res 512 --views 8 --steps 300]             | --torch-bake
FateAvatar's SECOND stage, neural baking, in feature-map mode (fateavatar_amd/bake.py: `BakeStep(texture="feature_map")`): the head
template's 65 536 UV-raster points + 65 536 template points, one [1,11,512,512] texture trained by the step's own fused Adam at 1e-3
towards frames rendered from a second random texture; L1 + the rot term at 0.1, every attribute baked: decode, frame, terms, decode
backward and Adam in ONE replayed graph.  --torch-bake: the A/B, the same loop through `BakedAvatar.render(return_values=True)` + the
torch rot term (tests/bake_ref.py: run it from a checkout that has tests/) + torch.optim.Adam, eager.  Prints steps/s and the image
loss at start and end.

    python tools/train_synthetic.py --rigged [--P 10006 --sh-degree 3 --binding-op]
GaussianAvatars' step (fateavatar_amd/rigged.py): Gaussians rigged to the triangles of the posed template, one GPU.
    python tools/train_synthetic.py --rigged --P 10006 --regularisers --densify-from 0.3 --densify-interval 0.1 --reset-interval 0.5
the same with the reference's scale / xyz regularisers in the step and a compressed maintenance schedule (fractions of
--steps: config/gaussianavatars.yaml:36-43 has 10 000 / 2 000 / 60 000 of 600 000 iterations); P and min(binding_counter)
are printed after each densify.
    python tools/train_synthetic.py --rigged --P 10006 --dssim [--regularisers]
the reference's image term, 0.8 x L1 + 0.2 x d_ssim (--image-loss RGB DSSIM for other weights; also for the generic step).

    python tools/train_synthetic.py --splatting [--P 10000 --binding-op | --torch-binding] [--reference-loss]
    python tools/train_synthetic.py --splatting --densify-from 0.3 --densify-interval 0.1 --reset-interval 0.5 --walk-interval 0.1
SplattingAvatar's step (fateavatar_amd/splatting.py): Gaussians on the Phong surface of the posed template, SH degree 0, one
GPU.  --torch-binding binds with the stock-PyTorch restatement (tests/phong_ref.py) in front of render(): the A/B.

    python tools/train_synthetic.py --flash [--P 16384 --binding-op | --torch-binding] [--mouth-mask] [--vertex-grad]
FlashAvatar's step (fateavatar_amd/flash.py): Gaussians at fixed barycentric points of the posed template, moved per frame by a
small torch deformation network (positional encoding of the canonical point + a per-frame condition, six hidden layers of 256,
ten outputs; torch.optim.Adam at 1e-4) that is trained through `step.d_deform`; Huber image term, SH degree 0, one GPU.
--torch-binding: binding and Huber as the stock-PyTorch restatement (tests/flash_ref.py) with autograd in front of render().
    python tools/train_synthetic.py --flash --fused-mlp [--P 16384] [--mouth-mask] [--vertex-grad]
The same loop with the deformation network INSIDE the captured step (fateavatar_amd/mlp.py: `FlashStep(deformer=DeformMLP(...))`,
the reference's embedding order and network shape, f32-MFMA kernels, a second fused Adam at 1e-4): one graph replay per step.

    python tools/train_synthetic.py --flash --lpips [--lpips-start 0] [--fused-mlp]       | --flash --torch-lpips
    python tools/train_synthetic.py --splatting --reference-loss --lpips                 | --splatting --reference-loss --torch-lpips
The reference's LPIPS term inside the step (`FlashStep(lpips=Lpips(.., weight=0.05))`, `SplattingStep(lpips=Lpips(.., weight=0.01))`):
one call behind the image-loss launch adds its gradient to the image gradient (csrc/fr_vgg.hip, fr_lpips_loss_grad) — the 13-layer
trunk at the frame's size, seeded weights.  --torch-lpips: the A/B, the same term at the same place through F.conv2d and autograd.
The report gains `lpips_loss` (the sum of the five tap terms, then the terms).

    python tools/train_synthetic.py --splatting --track-mesh [--track-offset 0.005 --track-lr 5e-4] [--binding-op | --torch-binding]
SplattingAvatar's step with the reference's tracking optimisation next to it (train/base.py:113-156), reduced to a rigid pose: every
frame's posed mesh gets an axis-angle and translation correction, a torch leaf of six numbers that starts --track-offset away
from the truth (zero) and is trained by torch Adam through `posed.backward(step.d_verts)` (`SplattingStep(mesh_grad=True)`).
Prints the mean pose error (vertex displacement) at the start and the end, and steps/s.

    python tools/train_synthetic.py --mono [--P 100000] [--torch-lbs]
MonoGaussianAvatar's loop (fateavatar_amd/mono.py): --P free points (default 100 000, the reference's max_points) with a torch
deformer network (four hidden layers of 128: expression basis, pose-corrective basis and skinning weights per point), a geometry
network (seven of 256) and a Gaussian network (two of 64), moved by a synthetic bone sequence through
deform_points -> splat_attributes -> render_points and trained on L1 + the three blendshape terms against per-vertex tables of
the template (nearest_vertex, lbs_terms_and_grad); torch.optim.Adam at 1e-4.  --torch-lbs: deformation, nearest vertex and the
three terms as the stock-PyTorch restatement (tests/mono_ref.py) with autograd and torch gathers: the A/B.  Like --torch-binding,
it imports the restatement from the test tree: run it from a checkout that has tests/, not from an installed package alone.
    python tools/train_synthetic.py --mono --track [--torch-lbs]
the same loop with the reference's tracking optimisation next to it (train/base.py:113-156): every frame's bones come from torch
leaves (axis-angle per bone -> Rodrigues -> `transforms` and `pose_feature`) and an expression vector, which start perturbed from
the truth and are trained by torch.optim.Adam(lr=5e-4) through deform_points(frame_grad=True); the JSON line gains the RMS error
of the axis-angles and of the expression against the truth at the start and at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
os.environ.setdefault("FR_TUNE_RUNTIME", "1")   # (fateavatar_amd.tune_runtime() at import: the runtime switches the measurements are quoted under)
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fateavatar_amd import dp, scenes  # noqa: E402
from fateavatar_amd.loss import ImageLoss  # noqa: E402
from fateavatar_amd.model import FlatGaussians, TorchCamera  # noqa: E402
from fateavatar_amd.render import render  # noqa: E402
from fateavatar_amd.train import TrainStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--lanes", dest="chain", action="store_false",
                    help="--views-per-step K: K lanes on K streams (a graph per frame) instead of ONE launch chain on one "
                         "stream (render_batch: the default)")
    ap.add_argument("--random-order", action="store_true",
                    help="FateAvatar step: area-weighted random binding points, stored as drawn, instead of the reference's "
                         "UV-raster initialisation (model/fateavatar.py:128-133)")
    ap.add_argument("--keep-coherent", action="store_true",
                    help="FateAvatar step: re-store the rows in a spatially coherent order after every densification (an "
                         "extension; the reference appends)")
    ap.add_argument("--binding-op", action="store_true",
                    help="FateAvatar step: the stand-alone binding kernels instead of the binding inside the rasterizer's kernels")
    ap.add_argument("--views-per-step", type=int, default=1,
                    help="--fateavatar: frames per optimisation step, rendered in flight together (the reference's batch)")
    ap.add_argument("--fateavatar", action="store_true",
                    help="FateAvatar's own loop: mesh-bound parameters (offset / rotation / scaling / colour / opacity), "
                         "synthetic INSTA-layout sequence with per-frame posed mesh, SH degree 0")
    ap.add_argument("--bake", action="store_true",
                    help="neural baking in feature-map mode: BakeStep(texture='feature_map') on the head template (one GPU)")
    ap.add_argument("--torch-bake", action="store_true",
                    help="the A/B of --bake: BakedAvatar.render + torch rot term + torch.optim.Adam, eager")
    ap.add_argument("--vertex-grad", action="store_true",
                    help="--fateavatar: AvatarStep(vertex_grad=True): every step leaves dLoss/dposed_verts in step.d_verts")
    ap.add_argument("--train-mesh", action="store_true",
                    help="--fateavatar: train a torch delta_vertex leaf under the Gaussians through step.d_verts, with the mesh terms")
    ap.add_argument("--mesh-terms", type=float, nargs=2, default=None, metavar=("LAP", "FLAME"),
                    help="--train-mesh: weights of the Laplacian and FLAME-distance terms (default: the reference's 1e5 0)")
    ap.add_argument("--mesh-lr", type=float, default=1e-4, help="--train-mesh: Adam rate of delta_vertex (train/optim.py:30)")
    ap.add_argument("--fused-flame", action="store_true",
                    help="--fateavatar: FLAME and its learnt deltas inside the captured step (AvatarStep(flame=FlameMesh), "
                         "fr_flame_forward / _backward and a second fused Adam), with the mesh terms")
    ap.add_argument("--torch-flame", action="store_true",
                    help="--fateavatar: the A/B of --fused-flame: the same loop with FLAME in stock PyTorch (tests/flame_ref.py) around "
                         "the step and torch.optim.Adam over the three deltas")
    ap.add_argument("--flame-shape", type=int, default=100, help="--fused-flame / --torch-flame: shape columns of the synthetic FLAME")
    ap.add_argument("--flame-exp", type=int, default=50, help="--fused-flame / --torch-flame: expression columns (1 .. 128)")
    ap.add_argument("--perceptual", action="store_true",
                    help="--fateavatar (plain loop, --fused-flame or --torch-flame): FateAvatar's VGG perceptual term at weight 0.1 inside "
                         "the step (AvatarStep(perceptual=Perceptual(VggFeatures.vgg16())), csrc/fr_vgg.hip); seeded random weights "
                         "unless --vgg-weights is given")
    ap.add_argument("--scale-term", action="store_true",
                    help="--fateavatar (any of its loops, any --views-per-step): FateAvatar's scale-ratio term at weight 0.1, threshold "
                         "9.0 inside the step (AvatarStep(scale_term=REFERENCE_SCALE_TERM), one launch in front of Adam); with "
                         "--fused-flame --perceptual the reference's whole objective; the report gains `reg_loss`")
    ap.add_argument("--torch-perceptual", action="store_true",
                    help="the A/B of --perceptual: the same term at the same place of the same loop through F.conv2d and autograd "
                         "(the reference's route, tools/loss_utils/vgg_feature.py)")
    ap.add_argument("--vgg-weights", default=None, metavar="FILE",
                    help="--perceptual / --torch-perceptual: a torch-saved state dict in torchvision's naming (vgg16().state_dict())")
    ap.add_argument("--perceptual-size", type=int, default=224, help="what both images are resized to (the reference: 224)")
    ap.add_argument("--lpips", action="store_true",
                    help="--flash, or --splatting --reference-loss: the reference's LPIPS term inside the step (FlashStep(lpips=Lpips(.., "
                         "weight=0.05), lpips_start=--lpips-start) / SplattingStep(lpips=Lpips(.., weight=0.01)), csrc/fr_vgg.hip's "
                         "fr_lpips_loss_grad); seeded random weights (pretrained ones are the caller's: Lpips.from_state_dicts)")
    ap.add_argument("--torch-lpips", action="store_true",
                    help="the A/B of --lpips: the same term at the same place of the same step through F.conv2d and autograd")
    ap.add_argument("--lpips-start", type=int, default=0,
                    help="--flash --lpips: the term is launched from this step + 1 on (the reference: 15000; default 0, so that the "
                         "timed loop carries it)")
    ap.add_argument("--track-camera", action="store_true",
                    help="--fateavatar: train a per-frame camera translation leaf through AvatarStep(camera_grad=True)")
    ap.add_argument("--track-offset", type=float, default=0.005, help="--track-camera: RMS start error of the translations, per axis (m)")
    ap.add_argument("--track-lr", type=float, default=5e-4, help="--track-camera: Adam rate (config/fateavatar.yaml:50 tracking_lr)")
    ap.add_argument("--track-mesh", action="store_true",
                    help="--splatting: every frame's posed mesh gets a rigid correction (axis-angle + translation, a torch leaf of "
                         "six numbers that starts --track-offset away), trained by torch Adam at --track-lr through "
                         "SplattingStep(mesh_grad=True)'s d_verts; with --torch-binding the same through stock PyTorch autograd")
    ap.add_argument("--rigged", action="store_true",
                    help="GaussianAvatars' loop: Gaussians bound to the local frames of the template's faces (one per face, then "
                         "random faces up to --P), rendered with --sh-degree active; --binding-op as for --fateavatar")
    ap.add_argument("--splatting", action="store_true",
                    help="SplattingAvatar's loop: --P Gaussians sampled on the template's Phong surface (default 10 000, the "
                         "reference's num_init_samples), SH degree 0; --binding-op as for --fateavatar")
    ap.add_argument("--reference-loss", action="store_true",
                    help="--splatting: the reference's objective without LPIPS, 1.0 x L1 + 10.0 x MSE + 1.0 x the scale term "
                         "(SplattingStep(image_loss=REFERENCE_IMAGE_LOSS, scale_term=REFERENCE_SCALE_TERM)); default: L1 alone")
    ap.add_argument("--torch-binding", action="store_true",
                    help="--splatting: the mesh pass and the binding in stock PyTorch (tests/phong_ref.py) in front of render(); "
                         "--flash: the binding and the Huber term in stock PyTorch (tests/flash_ref.py)")
    ap.add_argument("--flash", action="store_true",
                    help="FlashAvatar's loop: --P Gaussians (default 16 384, tex_size 128 squared) at fixed points of the template, "
                         "deformed per frame by a torch MLP trained through step.d_deform; Huber loss; --binding-op as for --fateavatar")
    ap.add_argument("--fused-mlp", action="store_true",
                    help="--flash: the deformation MLP runs inside the captured step (mlp.DeformMLP, fr_mlp_forward / _backward and "
                         "a second fused Adam) instead of stock PyTorch around it")
    ap.add_argument("--mono", action="store_true",
                    help="MonoGaussianAvatar's loop: --P free points (default 100 000) deformed by learned per-point linear blend "
                         "skinning, colours from a torch network, L1 + the three blendshape terms")
    ap.add_argument("--torch-lbs", action="store_true",
                    help="--mono: deformation, nearest vertex and blendshape terms in stock PyTorch (tests/mono_ref.py: needs the "
                         "checkout's tests/ next to tools/)")
    ap.add_argument("--track", action="store_true",
                    help="--mono: the frames' bones and expression are torch leaves (axis-angle per bone, an expression vector) that "
                         "start perturbed and are trained by Adam at 5e-4 through deform_points(frame_grad=True)")
    ap.add_argument("--mouth-mask", action="store_true",
                    help="--flash: every frame brings a mouth mask (the Huber term's second sum, weight 40)")
    ap.add_argument("--regularisers", action="store_true",
                    help="--rigged: the reference's scale / xyz regularisers in every step (one more launch in the graph)")
    ap.add_argument("--reg-weights", type=float, nargs=2, default=None, metavar=("SCALE", "XYZ"),
                    help="--rigged: regulariser weights (default 1.0 0.01); implies --regularisers")
    ap.add_argument("--reg-thresholds", type=float, nargs=2, default=None, metavar=("SCALE", "XYZ"),
                    help="--rigged: regulariser thresholds (default 0.6 1.0); implies --regularisers")
    ap.add_argument("--image-loss", type=float, nargs=2, default=None, metavar=("RGB", "DSSIM"),
                    help="--rigged and the generic step: the image term is RGB x L1 + DSSIM x d_ssim (two launches where the L1 "
                         "launch is); default: L1 with weight 1")
    ap.add_argument("--dssim", action="store_true", help="shorthand for --image-loss 0.8 0.2 (GaussianAvatars' and 3DGS's mix)")
    ap.add_argument("--densify-from", type=float, default=0.0,
                    help="--rigged / --splatting: first densify_and_prune at this fraction of --steps (0: no densification)")
    ap.add_argument("--densify-interval", type=float, default=0.1, help="--rigged / --splatting: densify every this fraction of --steps")
    ap.add_argument("--walk-interval", type=float, default=0.0,
                    help="--splatting: walk_on_triangles every this fraction of --steps (0: never)")
    ap.add_argument("--reset-interval", type=float, default=0.0,
                    help="--rigged / --splatting: reset_opacity every this fraction of --steps (0: never)")
    a = ap.parse_args()
    rank, world, local = dp.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    a.image_loss = ImageLoss(*a.image_loss) if a.image_loss else (ImageLoss(0.8, 0.2) if a.dssim else None)
    if a.reference_loss and (not a.splatting or a.torch_binding):
        raise SystemExit("--reference-loss goes with --splatting (and its fused terms: not with --torch-binding)")
    if a.bake or a.torch_bake:
        if (a.bake and a.torch_bake) or a.image_loss or a.fateavatar or a.rigged or a.splatting or a.flash or a.mono or world > 1:
            raise SystemExit("--bake / --torch-bake: one of the two, alone (L1 + the rot term), on one GPU")
        return main_bake(a, dev)
    if a.mono:
        if a.image_loss or a.train_mesh or a.mesh_terms or a.fateavatar or a.rigged or a.splatting or a.flash:
            raise SystemExit("--mono: the image term is L1 and there are no mesh terms; one model per run")
        return main_mono(a, rank, world, dev)
    if a.torch_lbs or a.track:
        raise SystemExit("--torch-lbs and --track go with --mono")
    if a.flash:
        if a.image_loss or a.train_mesh or a.mesh_terms or a.fateavatar or a.rigged or a.splatting:
            raise SystemExit("--flash: FlashAvatar's step has its own image term (Huber) and no mesh terms; one model per run")
        if a.fused_mlp and a.torch_binding:
            raise SystemExit("--fused-mlp: the fused step has no stock-PyTorch binding variant (drop --torch-binding)")
        return main_flash(a, rank, world, dev)
    if a.mouth_mask or a.fused_mlp:
        raise SystemExit("--mouth-mask and --fused-mlp go with --flash")
    if (a.train_mesh or a.vertex_grad or a.mesh_terms or a.track_camera) and not (a.fateavatar and a.views_per_step == 1):
        raise SystemExit("--train-mesh / --vertex-grad / --mesh-terms / --track-camera go with --fateavatar at one frame per step")
    if a.fused_flame or a.torch_flame:
        if not (a.fateavatar and a.views_per_step == 1) or (a.fused_flame and a.torch_flame) or a.train_mesh or a.track_camera:
            raise SystemExit("--fused-flame / --torch-flame: one of the two, with --fateavatar at one frame per step, without "
                             "--train-mesh / --track-camera")
    if a.perceptual or a.torch_perceptual:
        if not (a.fateavatar and a.views_per_step == 1) or (a.perceptual and a.torch_perceptual) or a.train_mesh or a.track_camera:
            raise SystemExit("--perceptual / --torch-perceptual: one of the two, with --fateavatar at one frame per step, without "
                             "--train-mesh / --track-camera")
    if a.lpips or a.torch_lpips:
        if (a.lpips and a.torch_lpips) or not (a.flash or (a.splatting and a.reference_loss)) or a.torch_binding or a.track_mesh:
            raise SystemExit("--lpips / --torch-lpips: one of the two, with --flash or --splatting --reference-loss, without "
                             "--torch-binding / --track-mesh")
    if a.track_mesh and not a.splatting:
        raise SystemExit("--track-mesh goes with --splatting")
    if a.scale_term and not a.fateavatar:
        raise SystemExit("--scale-term goes with --fateavatar (SplattingAvatar's own scale term: --splatting --reference-loss)")
    if a.fateavatar:
        if a.image_loss:
            raise SystemExit("--fateavatar: the D-SSIM term is not part of FateAvatar's objective (dssim_loss 0.0)")
        return main_fateavatar(a, rank, world, dev)
    if a.rigged:
        return main_rigged(a, rank, world, dev)
    if a.splatting:
        if a.image_loss:
            raise SystemExit("--splatting: the image term is L1, or with --reference-loss the reference's L1 + MSE (DESIGN.md)")
        return main_splatting(a, rank, world, dev)
    truth = scenes.head_scene(P=a.P, res=a.res, sh_degree=a.sh_degree, seed=0, opacity=0.5)
    cams = [TorchCamera(scenes.head_scene(P=8, res=a.res, sh_degree=a.sh_degree, seed=0, view=v, n_views=a.views).camera, dev)
            for v in range(a.views)]
    bg = torch.from_numpy(truth.bg).to(dev)
    pc_true = FlatGaussians(truth.means3D, truth.shs, truth.opacities, truth.scales, truth.rotations, a.sh_degree, dev,
                            fused_activations=True)
    with torch.no_grad():
        gts = [render(c, pc_true, bg)["render"].clone() for c in cams]
    rng = np.random.default_rng(1)
    shs0 = (truth.shs + 0.2 * rng.standard_normal(truth.shs.shape)).astype(np.float32)
    pc = FlatGaussians(truth.means3D, shs0, truth.opacities * 0.6, truth.scales, truth.rotations, a.sh_degree, dev,
                       fused_activations=True)
    cam = TorchCamera(scenes.head_scene(P=8, res=a.res, sh_degree=a.sh_degree, seed=0, view=0, n_views=a.views).camera, dev)
    ts = TrainStep(pc, cam, bg, use_graph=not a.no_graph, image_loss=a.image_loss)
    losses = []
    warm = 10
    for it in range(warm):
        v = (it * world + rank) % a.views
        losses.append(ts.step(cams[v], gts[v]).clone())
    torch.cuda.synchronize()
    dp.barrier()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        v = (it * world + rank) % a.views
        loss = ts.step(cams[v], gts[v])
        if it >= warm + a.steps - 4:     # (the loss lives in the step's static buffer: a trainer reads it now and then,
            losses.append(loss.clone())  # and a 4-byte device copy per step costs 14 us of a 180 us step)
    torch.cuda.synchronize()
    dp.barrier()
    dt = time.perf_counter() - t0
    ts.check()
    if rank == 0:
        l = [float(x) for x in losses]
        print(json.dumps({"metric": "optimisation steps/s (render + L1 + backward + stats + Adam)", "value": round(a.steps / dt, 1),
                          "frames_per_s": round(world * a.steps / dt, 1), "n_gpus": world, "ms_per_step": round(dt / a.steps * 1e3, 4),
                          "P": a.P, "res": a.res, "views": a.views, "graph": not a.no_graph,
                          "image_loss": list(a.image_loss) if a.image_loss else None,
                          "loss_first": round(float(np.mean(l[:4])), 6), "loss_last": round(float(np.mean(l[-4:])), 6)}))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def main_bake(a, dev):
    """--bake / --torch-bake: see the module docstring."""
    from fateavatar_amd import insta
    from fateavatar_amd.avatar import AvatarGaussians
    from fateavatar_amd.bake import BAKE_LR, REFERENCE_ROT_TERM, BakeStep
    from fateavatar_amd.baked import ATTRIBUTES, TEMPLATE_POINTS, BakedAvatar
    from fateavatar_amd.texture import SH_C0, TEXTURE_CHANNELS
    transform, posed, faces = insta.synthetic_sequence(a.views, a.res, 0)
    verts, _, _ = scenes.head_geometry()
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    posed, faces, canon = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(verts).to(dev)
    bg = torch.ones(3, device=dev)
    pc = AvatarGaussians.from_template(dev, uv_resolution=256)               # 65 536 points: the reference's tex_size 256
    baked = BakedAvatar(pc, tex_size=512, template_points=TEMPLATE_POINTS, rng=np.random.default_rng(0))
    gen = torch.Generator().manual_seed(1)
    # the targets: the frames of a second random texture (a step that owns no texture renders them)
    truth = torch.empty(1, 11, 512, 512).uniform_(-1, 1, generator=gen).to(dev)
    show = BakeStep(baked, faces, canon, cams[0].clone(), bg, use_graph=False)
    gts = []
    for v in range(a.views):
        show.step(cams[v], posed[v], torch.zeros(3, a.res, a.res, device=dev), truth)
        gts.append(show.out["render"].clone())
    st = BakeStep(baked, faces, canon, cams[0].clone(), bg, texture="feature_map", use_graph=not a.no_graph,
                  generator=torch.Generator().manual_seed(2))
    if a.torch_bake:
        from tests import bake_ref
        leaf = st.optim_texture.clone().requires_grad_(True)
        opt = torch.optim.Adam([leaf], lr=BAKE_LR)

        def step(v):
            td, off = {}, 0
            for name, c in TEXTURE_CHANNELS:
                td[name] = leaf[:, off:off + c]
                off += c
            td["color"] = torch.tanh(td["color"]) * (0.5 / SH_C0)
            outs, values = baked.render([cams[v]], [posed[v]], st.binding, bg, texture_dict=td, bake_attribute=ATTRIBUTES,
                                        return_values=True)
            l1 = torch.nn.functional.l1_loss(outs[0]["render"], gts[v])
            opt.zero_grad(set_to_none=True)
            (l1 + REFERENCE_ROT_TERM.weight * bake_ref.rot_loss(values["rotation"])).backward()
            opt.step()
            return l1.detach()
    else:
        step = lambda v: st.step(cams[v], posed[v], gts[v])  # noqa: E731
    losses, warm = [], 10
    for it in range(warm):
        losses.append(step(it % a.views).clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        loss = step(it % a.views)
        if it >= warm + a.steps - 4:
            losses.append(loss.clone())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if a.bake:
        st.check()
    l = [float(x) for x in losses]
    print(json.dumps({"metric": "neural-baking steps/s (decode + frame + L1 + rot term + backward + Adam, feature-map mode)",
                      "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4), "route": "torch" if a.torch_bake else "fused",
                      "points": baked.N, "texture": [11, 512, 512], "res": a.res, "views": a.views, "graph": bool(a.bake and not a.no_graph),
                      "loss_first": round(float(np.mean(l[:4])), 6), "loss_last": round(float(np.mean(l[-4:])), 6)}))


def make_perceptual(a, dev):
    """The step's perceptual term for --perceptual / --torch-perceptual (None without either): VGG-16's stack at weight 0.1 with
    the caller's weights (--vgg-weights) or seeded He-normal ones; --torch-perceptual: the same object with its one call
    replaced by the reference's route — stock convolutions and autograd — so that both variants sit at the same place of the
    same step."""
    if not (a.perceptual or a.torch_perceptual):
        return None
    import torch.nn.functional as F
    from fateavatar_amd.perceptual import Perceptual, VggFeatures
    size = (a.perceptual_size, a.perceptual_size)
    if a.vgg_weights:
        feats = VggFeatures.from_state_dict(torch.load(a.vgg_weights, map_location="cpu"), size=size, device=dev)
    else:
        rng = torch.get_rng_state()
        torch.manual_seed(0)
        feats = VggFeatures.vgg16(size=size, device=dev)
        torch.set_rng_state(rng)
    if a.perceptual:
        return Perceptual(feats, weight=0.1)

    m = torch.tensor(feats.mean, device=dev).view(1, 3, 1, 1)      # (made here: a captured step cannot copy from the host)
    s = torch.tensor(feats.std, device=dev).view(1, 3, 1, 1)

    class TorchPerceptual(Perceptual):
        def loss_and_grad(self, img, gt, loss_out=None, grad_out=None, accumulate=False, weight=None):
            f = self.features
            with torch.enable_grad():
                x = img.detach().requires_grad_(True)
                h = F.interpolate((torch.stack([x, gt]) - m) / s, mode="bilinear", size=f.size, align_corners=False)
                terms = []
                for y, w, b in zip(f.layers, f.weights, f.biases):
                    if y.pool_before:
                        h = F.max_pool2d(h, 2, 2)
                    h = F.relu(F.conv2d(h, w, b, padding=1))
                    if y.tap_after:
                        terms.append(F.l1_loss(h[0:1], h[1:2].detach()))
                total = torch.stack(terms).sum()
                (g,) = torch.autograd.grad(total, x)
            loss_out.copy_(torch.cat([total.detach().reshape(1), torch.stack(terms).detach()]))
            grad_out.add_(g, alpha=self.weight if weight is None else weight) if accumulate else grad_out.copy_(g * self.weight)
            return loss_out, grad_out
    return TorchPerceptual(feats, weight=0.1)


def make_lpips(a, dev, weight):
    """The step's LPIPS term for --lpips / --torch-lpips (None without either): the 13-layer trunk at the frame's size with seeded
    He-normal weights and uniform `lin`, at the objective's `weight`; --torch-lpips: the same object with its one call replaced
    by stock convolutions, the unit normalisation from stock ops and autograd, so that both sit at the same place of the step."""
    if not (a.lpips or a.torch_lpips):
        return None
    import torch.nn.functional as F
    from fateavatar_amd.perceptual import Lpips
    rng = torch.get_rng_state()
    torch.manual_seed(0)
    feats = Lpips.trunk((a.res, a.res), device=dev)
    torch.set_rng_state(rng)
    if a.lpips:
        return Lpips(feats, weight=weight)

    m = torch.tensor(feats.mean, device=dev).view(1, 3, 1, 1)      # (made here: a captured step cannot copy from the host)
    s = torch.tensor(feats.std, device=dev).view(1, 3, 1, 1)

    class TorchLpips(Lpips):
        def loss_and_grad(self, img, gt, loss_out=None, grad_out=None, accumulate=False, weight=None):
            f = self.features
            with torch.enable_grad():
                x = img.detach().requires_grad_(True)
                h = (torch.stack([x, gt]) - m) / s
                terms = []
                for y, w, b in zip(f.layers, f.weights, f.biases):
                    if y.pool_before:
                        h = F.max_pool2d(h, 2, 2)
                    h = F.relu(F.conv2d(h, w, b, padding=1))
                    if y.tap_after:
                        u = h / (h.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                        terms.append((self.lin[len(terms)].view(1, -1, 1, 1) * (u[0:1] - u[1:2].detach()).pow(2)).sum(1).mean())
                total = torch.stack(terms).sum()
                (g,) = torch.autograd.grad(total, x)
            loss_out.copy_(torch.cat([total.detach().reshape(1), torch.stack(terms).detach()]))
            grad_out.add_(g, alpha=self.weight if weight is None else weight) if accumulate else grad_out.copy_(g * self.weight)
            return loss_out, grad_out
    return TorchLpips(feats, weight=weight)


def fateavatar_setup(P, res, dev, views=8, views_per_step=1, use_graph=True, chain=True, fold_binding=True, order="uv",
                     keep_coherent=False, vertex_grad=False, mesh_terms=None, target_delta=None, camera_grad=False, perceptual=None,
                     scale_term=None):
    """FateAvatar's optimisation step on the synthetic INSTA-layout sequence: the mesh-bound Gaussian
    set, its step object (AvatarStep, or AvatarBatchStep for K > 1 frames per step), cameras, posed meshes and targets
    rendered from a hidden ground-truth set.  Used by this script and by bench.py's `avatar` mode.
    `vertex_grad`, `mesh_terms`, `camera_grad`: AvatarStep's options (K = 1); `scale_term`: both steps'.  `target_delta` [V,3] (numpy): the targets are rendered from
    the template displaced by it (`pose`, also returned, poses a displaced template differentiably).
    `order="uv"`: the reference's own initialisation — `uniform_sampling_barycoords(P, ...)` on the template's UV raster
    (model/fateavatar.py:128-133), rows in row-major texel order; `order="random"`: the area-weighted draw as drawn (the A/B)."""
    from fateavatar_amd import insta
    from fateavatar_amd.avatar import AvatarGaussians, AvatarStep, _BoundFrame
    from fateavatar_amd.binding import bind_gaussians
    n_frames = max(views, 8)
    transform, posed, faces = insta.synthetic_sequence(n_frames, res, seed=0)
    verts, _, _ = scenes.head_geometry()
    pc = AvatarGaussians.from_template(dev, num_points=P, sampling=order, rng=np.random.default_rng(0))
    fi, bc = pc.face_index.cpu().numpy(), pc.bary_coords.cpu().numpy()
    scale_init = float(pc._scaling[0, 0])
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    posed_t, faces_t, canon = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(verts).to(dev)
    bg = torch.ones(3, device=dev)
    wj, Rj, Rg = (torch.from_numpy(x).to(dev) for x in insta.synthetic_pose_maps(n_frames, seed=0))

    def pose(f, delta):
        """Frame f of the sequence for the template displaced by `delta` [V,3] (insta.synthetic_pose_maps): differentiable."""
        return posed_t[f] + ((1.0 - wj)[:, None] * delta + wj[:, None] * (delta @ Rj[f].T)) @ Rg[f].T

    # hidden ground truth: same binding, other appearance
    gt = AvatarGaussians(fi, bc, scale_init, dev)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(gt.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
        gt._offset.copy_((0.3 * torch.randn(gt.P, 1, generator=g)).to(dev))
    ref = AvatarStep(gt, faces_t, canon, TorchCamera(insta.camera_arrays(transform)[0], dev), bg, use_graph=False)
    gts = []
    with torch.no_grad():
        for f in range(n_frames):
            shown = posed_t[f] if target_delta is None else pose(f, torch.from_numpy(target_delta).to(dev)).contiguous()
            xyz, rot, scl = bind_gaussians(shown, ref.faces, gt.face_index, gt.bary_coords, ref.face_scale_canonical, gt._offset,
                                           gt._rotation, gt._scaling, ref.shell_len, True)
            gts.append(render(cams[f], _BoundFrame(xyz, gt, rot, scl, None), bg)["render"].clone())
    K = max(1, views_per_step)
    cam0 = TorchCamera(insta.camera_arrays(transform)[0], dev)
    if K == 1:
        extra = {}          # (only what is asked for: a plain run constructs the step exactly as before)
        if vertex_grad:
            extra["vertex_grad"] = True
        if mesh_terms is not None:
            extra["mesh_terms"] = mesh_terms
        if camera_grad:
            extra["camera_grad"] = True
        if perceptual is not None:
            extra["perceptual"] = perceptual
        if scale_term is not None:
            extra["scale_term"] = scale_term
        st = AvatarStep(pc, faces_t, canon, cam0, bg, use_graph=use_graph, fold_binding=fold_binding, keep_coherent=keep_coherent,
                        **extra)
    else:   # the reference's batch of K frames per step (model/fateavatar.py:251-276), in flight together
        from fateavatar_amd.avatar import AvatarBatchStep
        st = AvatarBatchStep(pc, faces_t, canon, cam0, bg, views_per_step=K, use_graph=use_graph, chain=chain,
                             fold_binding=fold_binding, keep_coherent=keep_coherent,
                             **({} if scale_term is None else {"scale_term": scale_term}))
    return dict(st=st, cams=cams, posed=posed_t, gts=gts, n_frames=n_frames, K=K, pose=pose, canon=canon,
                camera_arrays=insta.camera_arrays(transform))


def scale_term_of(a):
    """The step's scale term for --scale-term (None without it): the reference's 0.1 / 9.0."""
    if not a.scale_term:
        return None
    from fateavatar_amd.avatar import REFERENCE_SCALE_TERM
    return REFERENCE_SCALE_TERM


def reg_words(st):
    """`reg_loss` of a report: the step's unweighted scale_loss and the rows over the threshold (None without the term)."""
    return None if st.reg_loss is None else [round(float(st.reg_loss[0]), 6), int(st.reg_loss[1])]


def smooth_bump(verts, seed=0, height=0.004, width=0.03):
    """A seeded smooth displacement of the template [V,3] (numpy): three Gaussian bumps of `height` m and `width` m standard
    deviation around randomly chosen vertices of the face's front, along +z."""
    rng = np.random.default_rng(seed)
    front = np.flatnonzero((verts[:, 2] > 0.05) & (verts[:, 1] > 1.43))
    out = np.zeros_like(verts, dtype=np.float32)
    for c in verts[rng.choice(front, 3, replace=False)]:
        out[:, 2] += height * np.exp(-((verts - c) ** 2).sum(1) / (2 * width * width))
    return out


def main_train_mesh(a, rank, world, dev):
    """The demonstration of `step.d_verts`: FateAvatar's Gaussians by the fused step, its mesh by the caller's own Adam."""
    if world > 1 or a.views_per_step != 1:
        raise SystemExit("--train-mesh: one GPU, one frame per step (DESIGN.md)")
    from fateavatar_amd.loss import MeshTerms, REFERENCE_MESH_TERMS
    terms = MeshTerms(*a.mesh_terms) if a.mesh_terms else REFERENCE_MESH_TERMS
    verts, _, _ = scenes.head_geometry()
    bump = smooth_bump(np.asarray(verts, dtype=np.float32))
    su = fateavatar_setup(a.P, a.res, dev, views=a.views, use_graph=not a.no_graph, fold_binding=not a.binding_op,
                           order="random" if a.random_order else "uv", mesh_terms=terms, target_delta=bump,
                           scale_term=scale_term_of(a))
    st, cams, posed_t, gts, n_frames, pose = su["st"], su["cams"], su["posed"], su["gts"], su["n_frames"], su["pose"]
    bump_t = torch.from_numpy(bump).to(dev)
    delta = torch.zeros_like(bump_t, requires_grad=True)           # the reference's delta_vertex (model/fateavatar.py:93-94)
    opt = torch.optim.Adam([delta], lr=a.mesh_lr)                  # its `bs` group: the caller's, stock PyTorch

    def one_step(it):
        f = it % n_frames
        opt.zero_grad(set_to_none=True)
        posed = pose(f, delta)
        st.step(cams[f], posed, gts[f], verts_orig=posed_t[f])
        posed.backward(st.d_verts)                                 # dLoss/dposed_verts -> dLoss/ddelta through the motion
        opt.step()

    def report():
        torch.cuda.synchronize()
        return dict(image_loss=round(float(st.loss), 6), laplacian_loss=float(st.mesh_loss[0]), flame_loss=float(st.mesh_loss[1]),
                    delta_minus_bump=round(float((delta.detach() - bump_t).norm()), 6), reg_loss=reg_words(st))

    warm = 10
    one_step(0)
    first = report()
    for it in range(1, warm):
        one_step(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        one_step(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.check()
    print(json.dumps({"metric": "FateAvatar optimisation steps/s with the mesh trained (fused step + mesh terms + torch Adam on delta_vertex)",
                      "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4), "P": a.P, "res": a.res,
                      "frames": n_frames, "graph": not a.no_graph, "overflows": st.overflows, "mesh_terms": list(terms),
                      "mesh_lr": a.mesh_lr, "bump_norm": round(float(bump_t.norm()), 6), "first": first, "last": report()}))


def main_flame(a, rank, world, dev):
    """FateAvatar's whole iteration — the Gaussians AND the FLAME mesh under them with its three learnt deltas — with FLAME inside
    the captured step (--fused-flame) or as stock PyTorch around it (--torch-flame)."""
    if world > 1:
        raise SystemExit("--fused-flame / --torch-flame: one GPU (DESIGN.md)")
    from fateavatar_amd import flame
    from fateavatar_amd.avatar import AvatarGaussians, AvatarStep, _BoundFrame
    from fateavatar_amd.binding import bind_gaussians
    from fateavatar_amd.loss import MeshTerms, REFERENCE_MESH_TERMS
    terms = MeshTerms(*a.mesh_terms) if a.mesh_terms else REFERENCE_MESH_TERMS
    verts0, faces, _ = scenes.head_geometry()
    bump = smooth_bump(np.asarray(verts0, dtype=np.float32))
    verts = (verts0 - verts0.mean(0)).astype(np.float32)          # FLAME's own template sits at the origin
    n_frames = max(a.views, 8)
    fm = flame.synthetic_flame(verts, seed=0, n_shape=a.flame_shape, n_exp=a.flame_exp, device=dev)
    g = torch.Generator().manual_seed(3)
    frames = [flame.FlameFrame((0.5 * torch.randn(fm.n_exp, generator=g)).to(dev), (0.1 * torch.randn(15, generator=g)).to(dev))
              for _ in range(n_frames)]
    rng = np.random.default_rng(0)
    cams = []
    for _ in range(n_frames):
        eye = np.array([0.25 * rng.uniform(-1, 1), 0.15 * rng.uniform(-1, 1), 0.8 + 0.1 * rng.uniform(-1, 1)], np.float32)
        cams.append(TorchCamera(scenes.look_at_camera(eye, np.zeros(3), (0, 1, 0), 0.5, 0.5, a.res, a.res), dev))
    pc = AvatarGaussians.from_template(dev, num_points=a.P, sampling="random" if a.random_order else "uv", rng=np.random.default_rng(0))
    faces_t, canon, bg = torch.from_numpy(faces).to(dev), torch.from_numpy(verts).to(dev), torch.ones(3, device=dev)
    bump_t = torch.from_numpy(bump).to(dev)
    tables = (fm.v_template, fm.shapedirs, fm.posedirs, fm.J_regressor, fm.parents.cpu(), fm.lbs_weights, fm.n_shape)
    # hidden ground truth: same binding, other appearance, on the mesh whose delta_vertex is the bump
    gt = AvatarGaussians(pc.face_index.cpu().numpy(), pc.bary_coords.cpu().numpy(), float(pc._scaling.detach()[0, 0]), dev)
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(gt.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
        gt._offset.copy_((0.3 * torch.randn(gt.P, 1, generator=g)).to(dev))
    ref = AvatarStep(gt, faces_t, canon, cams[0].clone(), bg, use_graph=False)
    gts = []
    # (the targets are posed by the restatement in both modes, so that both train on the same images)
    from tests import flame_ref
    with torch.no_grad():
        for f in range(n_frames):
            shown = flame_ref.lbs(frames[f].expression, frames[f].pose, *tables, None, None, bump_t)[0].contiguous()
            xyz, rot, scl = bind_gaussians(shown, ref.faces, gt.face_index, gt.bary_coords, ref.face_scale_canonical, gt._offset,
                                           gt._rotation, gt._scaling, ref.shell_len, True)
            gts.append(render(cams[f], _BoundFrame(xyz, gt, rot, scl, None), bg)["render"].clone())
    common = dict(use_graph=not a.no_graph, fold_binding=not a.binding_op, mesh_terms=terms)
    if a.perceptual or a.torch_perceptual:
        common["perceptual"] = make_perceptual(a, dev)
    if a.scale_term:
        common["scale_term"] = scale_term_of(a)
    if a.fused_flame:
        st = AvatarStep(pc, faces_t, canon, cams[0].clone(), bg, flame=fm, **common)
        delta_vertex = lambda: fm.delta_vertex  # noqa: E731

        def one_step(it):
            f = it % n_frames
            st.step(cams[f], frames[f], gts[f])
    else:
        st = AvatarStep(pc, faces_t, canon, cams[0].clone(), bg, **common)
        sd = fm.state_dict()
        leaves = [sd[k].clone().requires_grad_(True) for k in flame.DELTA_KEYS]      # delta_shapedirs at its full [V,3,L]
        lrs = flame.REFERENCE_FLAME_LRS
        opt = torch.optim.Adam([{"params": [t], "lr": lrs[k]} for t, k in zip(leaves, flame.DELTA_KEYS)], lr=0.0)   # train/optim.py:27-33
        delta_vertex = lambda: leaves[2].detach()  # noqa: E731

        def one_step(it):
            f = it % n_frames
            opt.zero_grad(set_to_none=True)
            posed = flame_ref.lbs(frames[f].expression, frames[f].pose, *tables, *leaves)[0]     # model/fateavatar.py:212-218
            with torch.no_grad():
                orig = flame_ref.lbs(frames[f].expression, frames[f].pose, *tables)[0]           # :220-223
            st.step(cams[f], posed, gts[f], verts_orig=orig)
            posed.backward(st.d_verts)
            opt.step()

    def report():
        torch.cuda.synchronize()
        return dict(image_loss=round(float(st.loss), 6), laplacian_loss=float(st.mesh_loss[0]), flame_loss=float(st.mesh_loss[1]),
                    delta_minus_bump=round(float((delta_vertex() - bump_t).norm()), 6), reg_loss=reg_words(st))

    warm = 10
    one_step(0)
    first = report()
    for it in range(1, warm):
        one_step(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        one_step(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.check()
    how = "FLAME and both Adams inside the captured step" if a.fused_flame else "torch FLAME and torch Adam around the fused step"
    print(json.dumps({"metric": f"FateAvatar optimisation steps/s, Gaussians and FLAME deltas trained ({how})",
                      "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4), "P": a.P, "res": a.res,
                      "V": fm.V, "n_shape": fm.n_shape, "n_exp": fm.n_exp, "frames": n_frames, "graph": not a.no_graph,
                      "fused_flame": bool(a.fused_flame), "overflows": st.overflows, "mesh_terms": list(terms),
                      "perceptual": None if st.perceptual is None else ("torch" if a.torch_perceptual else "fused"),
                      "perceptual_loss": None if st.perceptual is None else [round(float(x), 6) for x in st.perceptual_loss],
                      "bump_norm": round(float(bump_t.norm()), 6), "first": first, "last": report()}))


def main_track_camera(a, rank, world, dev):
    """The demonstration of `step.d_view / d_proj / d_campos`: FateAvatar's Gaussians by the fused step, every frame's camera
    translation by the caller's own Adam (the reference's `train_cam_pose` embedding, which its rasterizer never moves)."""
    if world > 1 or a.train_mesh or a.mesh_terms:
        raise SystemExit("--track-camera: one GPU, without --train-mesh / --mesh-terms")
    from fateavatar_amd.model import PoseCamera
    su = fateavatar_setup(a.P, a.res, dev, views=a.views, use_graph=not a.no_graph, fold_binding=not a.binding_op,
                           order="random" if a.random_order else "uv", camera_grad=True, scale_term=scale_term_of(a))
    st, cams, posed_t, gts, n_frames = su["st"], su["cams"], su["posed"], su["gts"], su["n_frames"]
    arrays = su["camera_arrays"]
    # world_view_transform = [[R, 0], [T, 1]] (model.PoseCamera): the truth's rotation and translation of every frame
    Rs = [torch.from_numpy(np.ascontiguousarray(c.world_view_transform[:3, :3])).to(dev) for c in arrays]
    T_true = torch.from_numpy(np.stack([c.world_view_transform[3, :3] for c in arrays])).to(dev)
    g = torch.Generator().manual_seed(9)
    T = (T_true + a.track_offset * torch.randn(T_true.shape, generator=g).to(dev)).requires_grad_(True)   # the embedding's rows
    opt = torch.optim.Adam([T], lr=a.track_lr)
    shown = [c.clone() for c in cams]                                # per frame the camera block the step is handed

    def one_step(it):
        f = it % n_frames
        opt.zero_grad(set_to_none=True)
        c = arrays[f]
        cam = PoseCamera(Rs[f], T[f], c.FoVx, c.FoVy, (c.image_height, c.image_width))
        packed = torch.cat([cam.world_view_transform.reshape(-1), cam.full_proj_transform.reshape(-1), cam.camera_center])
        shown[f]._packed.copy_(packed.detach())
        st.step(shown[f], posed_t[f], gts[f])
        packed.backward(torch.cat([st.d_view.reshape(-1), st.d_proj.reshape(-1), st.d_campos]))
        opt.step()

    def report():
        torch.cuda.synchronize()
        return dict(image_loss=round(float(st.loss), 6), translation_rms_error=float((T.detach() - T_true).pow(2).mean().sqrt()),
                    reg_loss=reg_words(st))

    warm = 10
    one_step(0)
    first = report()
    for it in range(1, warm):
        one_step(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        one_step(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.check()
    print(json.dumps({"metric": "FateAvatar optimisation steps/s with the camera translations tracked (fused step with camera "
                                "gradients + torch Adam on the per-frame translation)",
                      "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4), "P": a.P, "res": a.res,
                      "frames": n_frames, "graph": not a.no_graph, "overflows": st.overflows, "track_lr": a.track_lr,
                      "track_offset": a.track_offset, "first": first, "last": report()}))


def main_fateavatar(a, rank, world, dev):
    if a.track_camera:
        return main_track_camera(a, rank, world, dev)
    if a.train_mesh:
        return main_train_mesh(a, rank, world, dev)
    if a.fused_flame or a.torch_flame:
        return main_flame(a, rank, world, dev)
    mesh_terms = moved = None
    if a.mesh_terms:       # the mesh terms in the plain loop (what the launch costs): a fixed displaced mesh held to the posed one
        from fateavatar_amd.loss import MeshTerms
        mesh_terms = MeshTerms(*a.mesh_terms)
    su = fateavatar_setup(a.P, a.res, dev, views=a.views, views_per_step=a.views_per_step, use_graph=not a.no_graph, chain=a.chain,
                           fold_binding=not a.binding_op, order="random" if a.random_order else "uv", keep_coherent=a.keep_coherent,
                           vertex_grad=a.vertex_grad, mesh_terms=mesh_terms, perceptual=make_perceptual(a, dev),
                           scale_term=scale_term_of(a))
    st, cams, posed_t, gts, n_frames, K = su["st"], su["cams"], su["posed"], su["gts"], su["n_frames"], su["K"]
    if mesh_terms is not None:
        bump = torch.from_numpy(smooth_bump(np.asarray(scenes.head_geometry()[0], dtype=np.float32))).to(dev)
        moved = [su["pose"](f, bump).contiguous() for f in range(n_frames)]

    def one_step(it, keep=True):
        if K == 1:
            f = (it * world + rank) % n_frames
            loss = st.step(cams[f], posed_t[f], gts[f]) if moved is None else st.step(cams[f], moved[f], gts[f], verts_orig=posed_t[f])
        else:
            fs = [((it * world + rank) * K + k) % n_frames for k in range(K)]
            loss = st.step([cams[f] for f in fs], [posed_t[f] for f in fs], [gts[f] for f in fs])[0]   # (first lane's loss)
        # the loss lives in the step's static buffer: a trainer reads it now and then (a 4-byte device copy per step costs
        # 14 us of a 180 us step)
        return loss.clone() if keep else None

    losses, warm = [], 10
    for it in range(warm):
        losses.append(one_step(it))
    torch.cuda.synchronize()
    dp.barrier()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        if it >= warm + a.steps - 4:
            losses.append(one_step(it))
        else:
            one_step(it, keep=False)
    t_host = time.perf_counter() - t0           # the host's share: everything enqueued
    torch.cuda.synchronize()
    dp.barrier()
    dt = time.perf_counter() - t0
    st.check()
    if rank == 0:
        l = [float(x) for x in losses]
        print(json.dumps({"host_enqueue_ms_per_step": round(t_host / a.steps * 1e3, 4),
                          "metric": "FateAvatar optimisation steps/s (bind + render + L1 + backward + stats + Adam)",
                          "storage_order": "random (area-weighted draw)" if a.random_order else "the reference's UV-raster initialisation (row-major texels)",
                          "binding": "stand-alone kernels" if a.binding_op else "inside the per-Gaussian kernels (fr_aux::binding)",
                          "value": round(a.steps / dt, 1), "frames_per_s": round(world * K * a.steps / dt, 1), "n_gpus": world,
                          "views_per_step": K, "launch_chain": bool(a.chain) if K > 1 else None,
                          "ms_per_step": round(dt / a.steps * 1e3, 4), "P": a.P, "res": a.res, "frames": n_frames, "sh_degree": 0,
                          "graph": not a.no_graph, "overflows": st.overflows, "vertex_grad": bool(st.vertex_grad) if K == 1 else False,
                          "mesh_terms": list(mesh_terms) if mesh_terms else None,
                          "mesh_loss": [float(x) for x in st.mesh_loss] if mesh_terms else None,
                          "perceptual": None if st.perceptual is None else ("torch" if a.torch_perceptual else "fused"),
                          "perceptual_loss": None if st.perceptual is None else [round(float(x), 6) for x in st.perceptual_loss],
                          "reg_loss": reg_words(st),
                          "loss_first": round(float(np.mean(l[:4])), 6), "loss_last": round(float(np.mean(l[-4:])), 6)}))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def rigged_setup(P, res, dev, views=8, sh_degree=3, use_graph=True, fold_binding=True, regularisers=None, image_loss=None):
    """GaussianAvatars' optimisation step on the synthetic INSTA-layout sequence: P Gaussians rigged to the template's faces
    (Gaussian i on face i for the first F = 10 006, the reference's initialisation; further ones on random faces, spread over
    them), the step object, cameras, posed meshes and targets rendered from a hidden ground-truth set of the same binding."""
    from fateavatar_amd import insta
    from fateavatar_amd.binding import bind_gaussians_face_local
    from fateavatar_amd.rigged import RiggedGaussians, RiggedStep, _RiggedFrame
    n_frames = max(views, 8)
    transform, posed, faces = insta.synthetic_sequence(n_frames, res, seed=0)
    F = int(faces.shape[0])
    rng = np.random.default_rng(0)
    binding = np.arange(min(P, F), dtype=np.int32)
    if P > F:
        binding = np.concatenate([binding, rng.integers(0, F, P - F).astype(np.int32)])
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    posed_t, faces_t = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev)
    bg = torch.ones(3, device=dev)
    g = torch.Generator().manual_seed(5)
    spread = (0.3 * torch.randn(len(binding), 3, generator=g) * torch.tensor([1.0, 0.1, 1.0])).to(dev)
    if P > F:   # several Gaussians per face: smaller, and not all on the face's centre
        spread[:F] = 0
    pc = RiggedGaussians(binding, dev)
    gt = RiggedGaussians(binding, dev)
    with torch.no_grad():
        for m in (pc, gt):
            if P > F:
                m._xyz.copy_(spread)
                m._scaling.fill_(float(np.log(max(F / P, 1e-3)) / 2))
            m.active_sh_degree = int(sh_degree)
        gt._features_dc.copy_((torch.rand(gt.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._features_rest.copy_((0.1 * torch.randn(gt.P, 15, 3, generator=g)).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
        gt._xyz.add_((0.1 * torch.randn(gt.P, 3, generator=g)).to(dev))
    gts = []
    with torch.no_grad():
        for f in range(n_frames):
            b = bind_gaussians_face_local(posed_t[f], faces_t.to(torch.int32), gt.binding, gt._xyz, gt._rotation, gt._scaling)
            gts.append(render(cams[f], _RiggedFrame(gt, None, b), bg)["render"].clone())
    st = RiggedStep(pc, faces_t, TorchCamera(insta.camera_arrays(transform)[0], dev), bg, posed_t[0], use_graph=use_graph,
                    fold_binding=fold_binding, regularisers=regularisers, image_loss=image_loss)
    return dict(st=st, cams=cams, posed=posed_t, gts=gts, n_frames=n_frames)


def main_rigged(a, rank, world, dev):
    if world > 1:
        raise SystemExit("--rigged: data-parallel runs are not built")
    from fateavatar_amd.rigged import REFERENCE_REGULARISERS, Regularisers
    reg = None
    if a.regularisers or a.reg_weights or a.reg_thresholds:
        reg = Regularisers(*(a.reg_weights or REFERENCE_REGULARISERS[:2]), *(a.reg_thresholds or REFERENCE_REGULARISERS[2:]))
    su = rigged_setup(a.P, a.res, dev, views=a.views, sh_degree=a.sh_degree, use_graph=not a.no_graph, fold_binding=not a.binding_op,
                      regularisers=reg, image_loss=a.image_loss)
    st, cams, posed_t, gts, n_frames = su["st"], su["cams"], su["posed"], su["gts"], su["n_frames"]
    # the compressed maintenance schedule, in steps of the timed loop (train/iteration.py:158-177)
    densify_from = int(round(a.densify_from * a.steps)) if a.densify_from > 0 else 0
    densify_every = max(1, int(round(a.densify_interval * a.steps)))
    reset_every = max(1, int(round(a.reset_interval * a.steps))) if a.reset_interval > 0 else 0
    gen = torch.Generator().manual_seed(0)
    losses, warm = [], 10
    for it in range(warm):
        losses.append(st.step(cams[it % n_frames], posed_t[it % n_frames], gts[it % n_frames]).clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        loss = st.step(cams[it % n_frames], posed_t[it % n_frames], gts[it % n_frames])
        if it >= warm + a.steps - 4:
            losses.append(loss.clone())
        k = it - warm + 1
        if densify_from and k >= densify_from and k < a.steps and (k - densify_from) % densify_every == 0:
            did = st.densify_and_prune(max_screen_size=20 if reset_every and k > reset_every else None, generator=gen)
            print(f"step {k}: cloned / split / pruned {did}, P {st.pc.P}, min binding_counter {int(st.binding_counter.min())}",
                  file=sys.stderr)
        if reset_every and k < a.steps and k % reset_every == 0:
            st.reset_opacity()
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.check()
    l = [float(x) for x in losses]
    print(json.dumps({"host_enqueue_ms_per_step": round(t_host / a.steps * 1e3, 4),
                      "metric": "GaussianAvatars optimisation steps/s (bind + render + L1 + backward + stats + Adam)",
                      "binding": "stand-alone kernels" if a.binding_op else "inside the per-Gaussian kernels (fr_aux::binding, face-local)",
                      "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4), "P": st.pc.P, "res": a.res,
                      "frames": n_frames, "sh_degree": st.pc.active_sh_degree, "graph": not a.no_graph, "overflows": st.overflows,
                      "regularisers": list(reg) if reg else None,
                      "image_loss": list(a.image_loss) if a.image_loss else None,
                      "loss_terms": [round(float(x), 6) for x in st.loss_terms] if a.image_loss else None,
                      "reg_loss": [round(float(x), 6) for x in st.reg_loss] if reg else None,
                      "loss_first": round(float(np.mean(l[:4])), 6), "loss_last": round(float(np.mean(l[-4:])), 6)}))


def splatting_setup(P, res, dev, views=8, use_graph=True, fold_binding=True, torch_binding=False, mesh_grad=False,
                    reference_loss=False, lpips=None):
    """SplattingAvatar's optimisation step on the synthetic INSTA-layout sequence (frame 0 is the canonical mesh): P Gaussians
    sampled on the template as the reference samples them, the step object, cameras, posed meshes and targets rendered from a
    hidden ground-truth set of the same embedding.  `reference_loss`: the step optimises the reference's L1 + MSE + scale term."""
    from fateavatar_amd import insta
    from fateavatar_amd.binding import bind_gaussians_phong, phong_canonical, phong_frame
    from fateavatar_amd.splatting import (REFERENCE_IMAGE_LOSS, REFERENCE_SCALE_TERM, SplattingGaussians, SplattingStep,
                                          _SplattingFrame)
    n_frames = max(views, 8)
    transform, posed, faces = insta.synthetic_sequence(n_frames, res, seed=0)
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    posed_t, faces_t = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev).to(torch.int32)
    canonical = phong_canonical(posed_t[0], faces_t)
    bg = torch.ones(3, device=dev)
    pc = SplattingGaussians.sample(posed_t[0], faces_t, P, torch.Generator().manual_seed(0))
    gt = SplattingGaussians(pc.face_index, pc.bary_coords, pc._scaling.detach()[:, 0], dev)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(gt.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
        gt._uvd[:, 2].copy_((0.002 * torch.randn(gt.P, generator=g)).to(dev))
        gt._rotation.add_((0.3 * torch.randn(gt.P, 4, generator=g)).to(dev))
        gt._scaling.add_((0.3 * torch.randn(gt.P, 3, generator=g)).to(dev))
    gts = []
    with torch.no_grad():
        for f in range(n_frames):
            b = bind_gaussians_phong(posed_t[f], faces_t, gt.face_index, gt.bary_coords, phong_frame(canonical, posed_t[f]),
                                     gt._uvd, gt._rotation, gt._scaling)
            gts.append(render(cams[f], _SplattingFrame(gt, None, b), bg)["render"].clone())
    cls = SplattingStep
    if torch_binding:
        from tests import phong_ref

        class TorchBoundStep(SplattingStep):
            """The A/B: the reference's own route — mesh pass and binding as stock PyTorch kernels in front of render().
            (R_posed R_cano^T instead of torch.inverse: the inverse does not capture into a graph.)"""
            def _forward_backward(self):
                pc, c = self.pc, self.canonical
                pc.begin_step()
                verts = self.verts.detach().requires_grad_(True) if self.mesh_grad else self.verts
                frame = phong_ref.mesh_frame(c.cano_verts, c.faces, verts, inverse=False)
                bound = phong_ref.phong_bind(verts, c.faces, pc.face_index, pc.bary_coords, frame, pc._uvd, pc._rotation,
                                             pc._scaling)
                out = render(self.cam, _SplattingFrame(pc, (self.xyz_gradient_accum, self.denom, pc.overflow_word), bound), self.bg)
                out["render"].backward(self._image_loss_and_grad(out["render"]))
                if self.mesh_grad:     # (float32 autograd through the restatement: the A/B of the two fused calls)
                    self.d_verts.copy_(verts.grad)
                pc.collect_grads()
                self.out = {"render": out["render"].detach(), "radii": out["radii"], "visibility_filter": out["visibility_filter"]}
        cls = TorchBoundStep
    st = cls(pc, canonical, TorchCamera(insta.camera_arrays(transform)[0], dev), bg, posed_t[0], use_graph=use_graph,
             fold_binding=fold_binding, mesh_grad=mesh_grad, image_loss=REFERENCE_IMAGE_LOSS if reference_loss else None,
             scale_term=REFERENCE_SCALE_TERM if reference_loss else None, lpips=lpips)
    return dict(st=st, cams=cams, posed=posed_t, gts=gts, n_frames=n_frames)


def main_track_mesh(a, rank, world, dev):
    """The demonstration of `SplattingStep(mesh_grad=True)`: SplattingAvatar's Gaussians by the fused step, every frame's rigid
    mesh correction by the caller's own Adam (the reference's per-frame tracking embeddings, train/base.py:113-156, reduced to a
    rigid pose: FLAME itself stays the caller's torch)."""
    if a.densify_from or a.walk_interval or a.reset_interval:
        raise SystemExit("--track-mesh: without the maintenance schedule (--densify-from / --walk-interval / --reset-interval)")
    P = a.P if "--P" in sys.argv else 10_000
    # (the restatement's matrix_to_quaternion indexes by a boolean mask while autograd records, as pytorch3d's does: a host
    # synchronisation, so the stock-PyTorch A/B cannot be captured and runs eagerly; compare it with --track-mesh --no-graph)
    use_graph = not a.no_graph and not a.torch_binding
    su = splatting_setup(P, a.res, dev, views=a.views, use_graph=use_graph, fold_binding=not a.binding_op,
                         torch_binding=a.torch_binding, mesh_grad=True, reference_loss=a.reference_loss)
    st, cams, posed_t, gts, n_frames = su["st"], su["cams"], su["posed"], su["gts"], su["n_frames"]
    g = torch.Generator().manual_seed(9)
    # per frame (axis-angle [rad], translation [m]) about the mesh's centroid; the truth is zero
    leaves = [(a.track_offset * torch.randn(6, generator=g)).to(dev).requires_grad_(True) for _ in range(n_frames)]
    opt = torch.optim.Adam(leaves, lr=a.track_lr)
    centres = posed_t.mean(dim=1, keepdim=True)

    def pose(f):
        w = leaves[f][:3]
        zero = w.new_zeros(())
        K = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
        return (posed_t[f] - centres[f]) @ torch.linalg.matrix_exp(K).T + centres[f] + leaves[f][3:]

    def one_step(it):
        f = it % n_frames
        opt.zero_grad(set_to_none=True)          # (a frame's leaf moves only in its own steps: Adam skips a leaf without a gradient)
        posed = pose(f)
        loss = st.step(cams[f], posed, gts[f])
        posed.backward(st.d_verts)
        opt.step()
        return loss

    def report():
        torch.cuda.synchronize()
        with torch.no_grad():
            all_leaves = torch.stack([l.detach() for l in leaves])
            err = torch.stack([(pose(f) - posed_t[f]).norm(dim=1).mean() for f in range(n_frames)]).mean()
        return dict(image_loss=round(float(st.loss), 6), mean_vertex_error_m=float(err),
                    rotation_rms_rad=float(all_leaves[:, :3].pow(2).mean().sqrt()),
                    translation_rms_m=float(all_leaves[:, 3:].pow(2).mean().sqrt()))

    first = dict(report(), image_loss=None)
    warm = 10
    for it in range(warm):
        one_step(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        one_step(it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.check()
    how = "stock PyTorch autograd (tests/phong_ref.py) in front of render()" if a.torch_binding else \
        "differentiable stand-alone ops" if a.binding_op else "fr_bind_backward_phong_frame + fr_phong_frame_backward behind the folded frame"
    last = report()
    print(f"mean pose error (vertex displacement): start {first['mean_vertex_error_m']:.6f} m, end {last['mean_vertex_error_m']:.6f} m; "
          f"{a.steps / dt:.1f} steps/s", file=sys.stderr)
    print(json.dumps({"metric": "SplattingAvatar optimisation steps/s with every frame's rigid mesh pose tracked (fused step with "
                                "mesh gradients + torch Adam on six numbers per frame)",
                      "vertex_gradient": how, "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4),
                      "P": st.pc.P, "res": a.res, "frames": n_frames, "graph": use_graph, "overflows": st.overflows,
                      "track_lr": a.track_lr, "track_offset": a.track_offset, "first": first, "last": last}))


def main_splatting(a, rank, world, dev):
    if world > 1:
        raise SystemExit("--splatting: data-parallel runs are not built")
    if a.track_mesh:
        return main_track_mesh(a, rank, world, dev)
    P = a.P if "--P" in sys.argv else 10_000
    su = splatting_setup(P, a.res, dev, views=a.views, use_graph=not a.no_graph, fold_binding=not a.binding_op,
                         torch_binding=a.torch_binding, reference_loss=a.reference_loss, lpips=make_lpips(a, dev, 0.01))
    st, cams, posed_t, gts, n_frames = su["st"], su["cams"], su["posed"], su["gts"], su["n_frames"]
    # the compressed maintenance schedule, in steps of the timed loop (config/splattingavatar.yaml:35-44,
    # train/iteration.py:271-298: densify every 100 steps from 600, reset opacity every 3 500, walk every 100)
    densify_from = int(round(a.densify_from * a.steps)) if a.densify_from > 0 else 0
    densify_every = max(1, int(round(a.densify_interval * a.steps)))
    reset_every = max(1, int(round(a.reset_interval * a.steps))) if a.reset_interval > 0 else 0
    walk_every = max(1, int(round(a.walk_interval * a.steps))) if a.walk_interval > 0 else 0
    gen = torch.Generator().manual_seed(0)
    losses, warm = [], 10
    for it in range(warm):
        losses.append(st.step(cams[it % n_frames], posed_t[it % n_frames], gts[it % n_frames]).clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        loss = st.step(cams[it % n_frames], posed_t[it % n_frames], gts[it % n_frames])
        if it >= warm + a.steps - 4:
            losses.append(loss.clone())
        k = it - warm + 1
        if densify_from and k >= densify_from and k < a.steps and (k - densify_from) % densify_every == 0:
            did = st.densify_and_prune(max_screen_size=20 if reset_every and k > reset_every else None, generator=gen)
            print(f"step {k}: cloned / split / pruned {did}, P {st.pc.P}, split {did[1]}, fit iterations {st.last_fit_iterations}",
                  file=sys.stderr)
        if walk_every and k < a.steps and k % walk_every == 0:
            st.walk_on_triangles()
        if reset_every and k < a.steps and k % reset_every == 0:
            st.reset_opacity()
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.check()
    l = [float(x) for x in losses]
    how = "stock PyTorch in front of render()" if a.torch_binding else "stand-alone kernels" if a.binding_op else \
        "mesh pass + inside the per-Gaussian kernels (fr_aux::binding, Phong surface)"
    terms = {}
    if a.reference_loss:     # the last step's words: (weighted image loss, l1, mse) and (scale_loss, rows it averaged over)
        lt, rl = [float(x) for x in st.loss_terms], [float(x) for x in st.reg_loss]
        terms = {"l1": round(lt[1], 6), "mse": round(lt[2], 6), "scale_loss": round(rl[0], 6), "scale_selected": int(rl[1])}
        print(f"last step: l1 {lt[1]:.6f}, mse {lt[2]:.6f}, scale_loss {rl[0]:.6f} over {int(rl[1])} selected rows", file=sys.stderr)
    objective = "L1 + MSE + scale term" if a.reference_loss else "L1"
    if st.lpips is not None:
        objective += " + 0.01 LPIPS"
        terms["lpips"] = "torch" if a.torch_lpips else "fused"
        terms["lpips_loss"] = [round(float(x), 6) for x in st.lpips_loss]
    print(json.dumps({"host_enqueue_ms_per_step": round(t_host / a.steps * 1e3, 4),
                      "metric": f"SplattingAvatar optimisation steps/s (mesh pass + bind + render + {objective} + backward + stats + Adam)",
                      "reference_loss": bool(a.reference_loss), **terms,
                      "binding": how, "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4), "P": st.pc.P,
                      "res": a.res, "frames": n_frames, "graph": not a.no_graph, "overflows": st.overflows,
                      "loss_first": round(float(np.mean(l[:4])), 6), "loss_last": round(float(np.mean(l[-4:])), 6)}))


class DeformNet(torch.nn.Module):
    """A deformation network of FlashAvatar's kind: the canonical point, identity plus sin / cos at the eight octave-spaced
    frequencies 2^0 .. 2^7 (3 + 48 inputs), concatenated with the frame's condition vector; six hidden layers of 256 with ReLU;
    ten outputs (the step applies tanh).  The last layer starts small, so the first frames are the undeformed avatar."""

    def __init__(self, points: torch.Tensor, cond_dim: int, hidden: int = 256, layers: int = 6):
        super().__init__()
        freqs = 2.0 ** torch.arange(8, dtype=torch.float32, device=points.device)
        ang = points[:, None, :] * freqs[None, :, None]                                   # [N,8,3]
        self.register_buffer("embedded", torch.cat([points, torch.sin(ang).flatten(1), torch.cos(ang).flatten(1)], dim=1))
        dims = [self.embedded.shape[1] + cond_dim] + [hidden] * layers
        mods = []
        for i, o in zip(dims[:-1], dims[1:]):
            mods += [torch.nn.Linear(i, o), torch.nn.ReLU()]
        self.net = torch.nn.Sequential(*mods, torch.nn.Linear(hidden, 10))
        with torch.no_grad():
            self.net[-1].weight.mul_(0.01)
            self.net[-1].bias.zero_()

    def forward(self, cond: torch.Tensor) -> torch.Tensor:
        return self.net(torch.cat([self.embedded, cond.expand(self.embedded.shape[0], -1)], dim=1))


def flash_setup(P, res, dev, views=8, use_graph=True, fold_binding=True, torch_binding=False, mouth_mask=False, vertex_grad=False,
                fused_mlp=False, lpips=None, lpips_start=0):
    """FlashAvatar's optimisation step on the synthetic INSTA-layout sequence: P Gaussians at fixed points of the template (the
    reference's UV-raster sampling when P is its row count, else uniform faces), the step object, the deformation network with
    its per-frame conditions (the frame's jaw and rigid rotations, from the sequence), cameras, posed meshes, mouth masks and
    targets rendered from a hidden ground-truth set at the same places with a per-frame deformation of its own.
    `fused_mlp`: `net` is a mlp.DeformMLP (the reference's embedding order; six hidden layers of 256; the last layer starts small
    like DeformNet's) and part of the step."""
    from fateavatar_amd import insta
    from fateavatar_amd.binding import bind_gaussians_deform
    from fateavatar_amd.flash import FlashGaussians, FlashStep, _FlashFrame
    from fateavatar_amd.knn import init_scale_by_knn
    from fateavatar_amd.splatting import sample_bary_on_triangles
    n_frames = max(views, 8)
    transform, posed, faces = insta.synthetic_sequence(n_frames, res, seed=0)
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    posed_t, faces_t = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev).to(torch.int32)
    canon = torch.from_numpy(np.asarray(scenes.head_geometry()[0], dtype=np.float32)).to(dev)
    bg = torch.ones(3, device=dev)
    g = torch.Generator().manual_seed(0)
    fi, bary = sample_bary_on_triangles(int(faces.shape[0]), P, g)
    pts = torch.einsum("nij,ni->nj", canon[faces_t.long()][fi.to(dev)], bary.to(dev)).contiguous()
    scale_init = float(init_scale_by_knn(pts)[2])
    pc, gt = FlashGaussians(fi, bary, scale_init, dev), FlashGaussians(fi, bary, scale_init, dev)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
        gt._rotation.add_((0.3 * torch.randn(P, 4, generator=g)).to(dev))
    _, Rj, Rg = insta.synthetic_pose_maps(n_frames, seed=0)
    conds = [torch.from_numpy(np.concatenate([Rj[f].reshape(-1), Rg[f].reshape(-1)])).to(dev) for f in range(n_frames)]
    # the hidden avatar's own deformation: smooth in the canonical point, different per frame
    gts, masks = [], []
    yy, xx = torch.meshgrid(torch.arange(res, device=dev), torch.arange(res, device=dev), indexing="ij")
    width = torch.tensor([0.002] * 3 + [0.3] * 4 + [0.2] * 3, device=dev)
    with torch.no_grad():
        for f in range(n_frames):
            phase = torch.linspace(0.0, 3.0, 10, device=dev) + f
            hidden = torch.sin(40.0 * pts.sum(1, keepdim=True) + phase) * width
            b = bind_gaussians_deform(posed_t[f], faces_t, gt.face_index, gt.bary_coords, hidden, gt._rotation, gt._scaling)
            gts.append(render(cams[f], _FlashFrame(gt, None, bound=b), bg)["render"].clone())
            masks.append((((yy - 0.62 * res) / (0.10 * res)) ** 2 + ((xx - 0.5 * res) / (0.16 * res)) ** 2 < 1).float()[None].contiguous())
    extra = {}
    if fused_mlp:
        from fateavatar_amd.mlp import DeformMLP, embed_points
        net = DeformMLP(embed_points(pc.canonical_points(canon, faces_t)).contiguous(), conds[0].numel(), layers=6)
        with torch.no_grad():
            net.weight(net.layers).mul_(0.01)
            net.bias(net.layers).zero_()
        extra = dict(deformer=net, deformer_lr=1e-4)
    else:
        net = DeformNet(pc.canonical_points(canon, faces_t), conds[0].numel()).to(dev)
    cls = FlashStep
    if torch_binding:
        from tests import flash_ref

        class TorchBoundStep(FlashStep):
            """The A/B: the reference's own route — binding and Huber term as stock PyTorch kernels with autograd around render()."""
            def _forward_backward(self):
                pc = self.pc
                pc.begin_step()
                verts = self._vertex_leaf(self.verts)
                deform = self.deform.detach().requires_grad_(True)
                bound = flash_ref.deform_bind(verts, self.faces, pc.face_index, pc.bary_coords, deform, pc._rotation, pc._scaling)
                out = render(self.cam, _FlashFrame(pc, (self.xyz_gradient_accum, self.denom, pc.overflow_word), bound=bound), self.bg)
                terms = flash_ref.huber_loss(out["render"], self.gt, self.mask, self.huber.alpha, self.huber.mask_weight)
                self.loss_terms.copy_(torch.stack([t.detach() for t in terms]))
                terms[0].backward()
                pc.collect_grads()
                self._keep_vertex_grad(verts)
                self.d_deform = deform.grad
                self.out = self._kept(out)
        cls = TorchBoundStep
    st = cls(pc, faces_t, TorchCamera(insta.camera_arrays(transform)[0], dev), bg, posed_t[0], use_graph=use_graph,
             fold_binding=fold_binding, mouth_mask=mouth_mask, vertex_grad=vertex_grad, lpips=lpips, lpips_start=lpips_start, **extra)
    return dict(st=st, net=net, conds=conds, cams=cams, posed=posed_t, gts=gts, masks=masks, n_frames=n_frames)


def main_flash(a, rank, world, dev):
    if world > 1:
        raise SystemExit("--flash: data-parallel runs are not built")
    P = a.P if "--P" in sys.argv else 16_384
    su = flash_setup(P, a.res, dev, views=a.views, use_graph=not a.no_graph, fold_binding=not a.binding_op,
                     torch_binding=a.torch_binding, mouth_mask=a.mouth_mask, vertex_grad=a.vertex_grad, fused_mlp=a.fused_mlp,
                     lpips=make_lpips(a, dev, 0.05), lpips_start=a.lpips_start)
    st, net, conds, cams, posed_t, gts, masks, n_frames = (su[k] for k in ("st", "net", "conds", "cams", "posed", "gts", "masks", "n_frames"))
    # the reference's `deformer` group (train/optim.py:55-59); with --fused-mlp the step's own second Adam
    opt = None if a.fused_mlp else torch.optim.Adam(net.parameters(), lr=1e-4)
    first = [p.detach().clone() for p in net.parameters()]

    def one_step(it):
        f = it % n_frames
        if a.fused_mlp:                                    # everything is in the step: one graph replay
            return st.step(cams[f], posed_t[f], conds[f], gts[f], masks[f] if a.mouth_mask else None)
        deform = net(conds[f])
        loss = st.step(cams[f], posed_t[f], deform, gts[f], masks[f] if a.mouth_mask else None)
        opt.zero_grad(set_to_none=True)
        deform.backward(st.d_deform)                       # dLoss/d(deform) -> the network's weights: stock PyTorch
        opt.step()
        return loss

    losses, warm = [], 10
    for it in range(warm):
        losses.append(one_step(it).clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        loss = one_step(it)
        if it >= warm + a.steps - 4:
            losses.append(loss.clone())
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.check()
    l = [float(x) for x in losses]
    how = "stock PyTorch (binding + Huber + autograd) around render()" if a.torch_binding else "stand-alone kernels" if a.binding_op else \
        "inside the per-Gaussian kernels (fr_aux::binding, MLP-deformed)"
    moved = max(float((p.detach() - q).abs().max()) for p, q in zip(net.parameters(), first))
    print(json.dumps({"host_enqueue_ms_per_step": round(t_host / a.steps * 1e3, 4),
                      "metric": "FlashAvatar optimisation steps/s (fused MLP + bind + render + Huber + backward + stats + Adam + MLP backward + MLP Adam, one graph)"
                      if a.fused_mlp else
                      "FlashAvatar optimisation steps/s (torch MLP + bind + render + Huber + backward + stats + Adam + MLP backward / Adam)",
                      "mlp": "fused (fr_mlp, inside the step)" if a.fused_mlp else "stock PyTorch", "binding": how, "value": round(a.steps / dt, 1), "ms_per_step": round(dt / a.steps * 1e3, 4), "P": st.pc.P,
                      "res": a.res, "frames": n_frames, "graph": not a.no_graph, "overflows": st.overflows,
                      "mouth_mask": bool(a.mouth_mask), "vertex_grad": bool(st.vertex_grad),
                      "lpips": None if st.lpips is None else ("torch" if a.torch_lpips else "fused"),
                      "lpips_loss": None if st.lpips is None else [round(float(x), 6) for x in st.lpips_loss],
                      "loss_terms": [round(float(x), 6) for x in st.loss_terms], "mlp_weights_moved": moved,
                      "loss_first": round(float(np.mean(l[:4])), 6), "loss_last": round(float(np.mean(l[-4:])), 6)}))


def _mlp(d_in, hidden, d_out):
    layers, d = [], d_in
    for h in hidden:
        layers += [torch.nn.Linear(d, h), torch.nn.Softplus(beta=100)]
        d = h
    return torch.nn.Sequential(*layers, torch.nn.Linear(d, d_out))


def main_mono(a, rank, world, dev):
    if world > 1:
        raise SystemExit("--mono: data-parallel runs are not built")
    from fateavatar_amd import mono
    if a.torch_lbs:
        from tests import mono_ref
    N, E, J, n_frames = a.P, 50, 6, a.views
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    rn = lambda *sh: torch.randn(sh, generator=gen)  # noqa: E731
    truth = scenes.head_scene(P=N, res=a.res, sh_degree=0, seed=0, opacity=0.5)
    cam = TorchCamera(truth.camera, dev)
    bg = torch.zeros(3, device=dev)
    # per-vertex tables of the template in fr_lbs_terms' layouts (FLAME's own are absent: smooth functions of the vertex)
    verts = torch.from_numpy(np.asarray(scenes.head_geometry()[0], np.float32))
    V, centre = verts.shape[0], verts.mean(0)
    rel = (verts - centre) / 0.15
    proj = lambda d: rel @ rn(3, d)  # noqa: E731
    gt_w = torch.softmax(2 * proj(J), 1)
    gt_P, gt_S = 0.003 * torch.tanh(proj(108)).reshape(V, 36, 3), 0.003 * torch.tanh(proj(3 * E)).reshape(V, 3, E)
    verts, gt_w, gt_P, gt_S = (t.contiguous().to(dev) for t in (verts, gt_w, gt_P, gt_S))

    def bones(angle):                     # rigid motions about the head's centre; bone 0 (the ghost bone) the identity
        r = angle * rn(J, 3)
        th = r.norm(dim=1).clamp_min(1e-12)
        k = r / th[:, None]
        K = torch.zeros(J, 3, 3)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
        R = torch.eye(3)[None] + torch.sin(th)[:, None, None] * K + (1 - torch.cos(th))[:, None, None] * (K @ K)
        A = torch.eye(4).repeat(J, 1, 1)
        A[:, :3, :3], A[:, :3, 3] = R, 0.004 * rn(J, 3) + centre - R @ centre
        A[0] = torch.eye(4)
        return A

    state = lambda angle, amp: mono.PoseState(*[t.to(dev) for t in (amp * rn(E), 0.3 * amp * rn(36), bones(angle))])  # noqa: E731
    canonical = state(0.02, 0.0)
    if a.track:
        # a frame's pose state as a differentiable function of its leaves: bone 0 the identity, bones 1 .. 4 give the pose feature
        centre_d, eye3 = centre.to(dev), torch.eye(3, device=dev)
        last_row = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).expand(J, 1, 4)

        def frame_state(r, expr, trans):
            th = r.norm(dim=1).clamp_min(1e-12)
            k, zero = r / th[:, None], torch.zeros_like(th)
            K = torch.stack([zero, -k[:, 2], k[:, 1], k[:, 2], zero, -k[:, 0], -k[:, 1], k[:, 0], zero], 1).reshape(J, 3, 3)
            R = eye3[None] + torch.sin(th)[:, None, None] * K + (1 - torch.cos(th))[:, None, None] * (K @ K)
            R = torch.cat([eye3[None], R[1:]], 0)
            t = torch.cat([torch.zeros((1, 3), device=dev), (trans + centre_d - R @ centre_d)[1:]], 0)
            A = torch.cat([torch.cat([R, t[:, :, None]], 2), last_row], 1)
            return mono.PoseState(expr, (R[1:5] - eye3[None]).reshape(36), A)

        r_true, expr_true, trans = (t.to(dev) for t in (0.12 * rn(n_frames, J, 3), 0.5 * rn(n_frames, E), 0.004 * rn(n_frames, J, 3)))
        with torch.no_grad():
            frames = [mono.PoseState(*[t.contiguous() for t in frame_state(r_true[f], expr_true[f], trans[f])]) for f in range(n_frames)]
        r_leaf = (r_true + 0.02 * rn(n_frames, J, 3).to(dev)).requires_grad_(True)
        expr_leaf = (expr_true + 0.1 * rn(n_frames, E).to(dev)).requires_grad_(True)
        opt_track = torch.optim.Adam([r_leaf, expr_leaf], lr=5e-4)       # tracking_lr (train/base.py:113-156)
        rms = lambda d: float(d.detach().pow(2).mean().sqrt())  # noqa: E731
        track_err = lambda: (rms((r_leaf - r_true)[:, 1:]), rms(expr_leaf - expr_true))  # noqa: E731
        err_first = track_err()
    else:
        frames = [state(0.12, 0.5) for _ in range(n_frames)]
    # targets: the hidden points carry their nearest vertex' table rows and fixed attributes
    pts_true = torch.from_numpy(np.asarray(truth.means3D, np.float32)).to(dev)
    feats_true = torch.cat([rn(N, 3), rn(N, 3) - 1.0, rn(N, 4), rn(N, 1)], 1).to(dev)
    radius = 0.002
    with torch.no_grad():
        idx = mono.nearest_vertex(pts_true, verts)[0].long()
        attrs = mono.splat_attributes(feats_true, torch.zeros_like(feats_true), radius, scene_scale=4.0)
        gts = [mono.render_points(cam, mono.deform_points(pts_true, gt_S[idx], gt_P[idx], gt_w[idx], canonical, f), *attrs, bg)[0].clone()
               for f in frames]
    points = (pts_true + 0.002 * rn(N, 3).to(dev)).requires_grad_(True)
    deformer, geometry, gaussian = _mlp(3, [128] * 4, 3 * E + 108 + J).to(dev), _mlp(3, [256] * 7, 11).to(dev), _mlp(3, [64, 64], 11).to(dev)
    nets = (deformer, geometry, gaussian)
    opt = torch.optim.Adam([points] + [p for n in nets for p in n.parameters()], lr=1e-4)
    terms = mono.reference_lbs_weights(10.0)
    lbs = torch.zeros(3, device=dev)

    def one_step(it):
        frame = frames[it % n_frames]
        opt.zero_grad(set_to_none=True)
        if a.track:
            opt_track.zero_grad(set_to_none=True)
            f = it % n_frames
            frame = frame_state(r_leaf[f], expr_leaf[f], trans[f])
        q = deformer((points.detach() - centre.to(dev)) / 0.15)
        S, P, w = 0.01 * q[:, :3 * E].reshape(N, 3, E), 0.01 * q[:, 3 * E:3 * E + 108].reshape(N, 36, 3), torch.softmax(q[:, 3 * E + 108:], 1)
        if a.torch_lbs:
            xyz = mono_ref.deform_points(points, S, P, w, canonical, frame)
        else:
            leaves = [t.detach().requires_grad_(True) for t in (S, P, w)]
            xyz = mono.deform_points(points, *leaves, canonical, frame, frame_grad=a.track)
        feats = geometry((points.detach() - centre.to(dev)) / 0.15)
        offs = gaussian((xyz.detach() - points.detach()) / 0.15)
        rgb, opacity, scales, rotations = mono.splat_attributes(feats, offs, radius, scene_scale=4.0)
        image = mono.render_points(cam, xyz, rgb, opacity, scales, rotations, bg)[0]
        loss = (image - gts[it % n_frames]).abs().mean()
        if a.torch_lbs:
            index = mono_ref.nearest_vertex(points.detach(), verts)[0]
            three = mono_ref.lbs_terms(index, w, P, S, gt_w, gt_P, gt_S)
            (loss + (three * torch.tensor(tuple(terms), device=dev)).sum()).backward()
            lbs.copy_(three.detach())
        else:
            loss.backward()                # image term -> points, the two attribute networks and the three leaves
            index = mono.nearest_vertex(points.detach(), verts)[0]
            mono.lbs_terms_and_grad(index, leaves[2], leaves[1], leaves[0], gt_w, gt_P, gt_S, terms, leaves[2].grad, leaves[1].grad,
                                    leaves[0].grad, out=lbs)
            torch.autograd.backward([S, P, w], [t.grad for t in leaves])      # -> the deformer's weights: stock PyTorch
        opt.step()
        if a.track:
            opt_track.step()
        return loss.detach()

    losses, warm = [], 5
    for it in range(warm):
        losses.append(one_step(it).clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(warm, warm + a.steps):
        loss = one_step(it)
        if it >= warm + a.steps - 4:
            losses.append(loss.clone())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    l = [float(x) for x in losses]
    tracked = {}
    if a.track:
        err_last = track_err()
        tracked = {"track": "axis-angle and expression leaves, torch.optim.Adam(lr=5e-4) through " +
                            ("autograd" if a.torch_lbs else "fr_point_lbs_backward_pose"),
                   "pose_err_first": err_first[0], "pose_err_last": err_last[0], "expression_err_first": err_first[1],
                   "expression_err_last": err_last[1]}
    print(json.dumps({**tracked,
                      "metric": "MonoGaussianAvatar optimisation steps/s (three torch MLPs + LBS + render + L1 + blendshape terms + "
                                "backward + Adam)",
                      "lbs": "stock PyTorch (tests/mono_ref.py)" if a.torch_lbs else "fused (fr_point_lbs, fr_nearest_vertex, fr_lbs_terms)",
                      "value": round(a.steps / dt, 2), "ms_per_step": round(dt / a.steps * 1e3, 3), "P": N, "V": V, "res": a.res,
                      "frames": n_frames, "lbs_terms": [float(x) for x in lbs],
                      "loss_first": round(float(np.mean(l[:4])), 6), "loss_last": round(float(np.mean(l[-4:])), 6)}))


if __name__ == "__main__":
    main()
