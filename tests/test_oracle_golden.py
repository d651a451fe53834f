"""CPU: pin the oracle (and the host-side camera helpers) against golden vectors produced by the
reference's own importable Python (tests/golden/make_golden.py)."""
import os

import numpy as np

from fateavatar_amd import scenes
from oracle import oracle

G = os.path.join(os.path.dirname(__file__), "golden")


def test_sh_colour_matches_reference_eval_sh():
    z = np.load(os.path.join(G, "golden_sh.npz"))
    dirs, sh = z["dirs"], z["sh"]
    campos = np.zeros(3, np.float32)
    worst = 0.0
    for deg in range(4):
        ref = np.maximum(z[f"deg{deg}"] + 0.5, 0.0)  # forward.cu:63-70 adds 0.5 and clamps
        for i in range(dirs.shape[0]):
            got, cl = oracle.eval_sh(deg, sh[i], dirs[i] * 2.5, campos)  # any point along the direction
            worst = max(worst, float(np.abs(got - ref[i]).max()))
            assert np.array_equal(cl, (z[f"deg{deg}"][i] + 0.5) < 0) or np.abs(z[f"deg{deg}"][i] + 0.5).min() < 1e-6
    assert worst < 2e-6, worst


def test_cov3d_matches_reference_build_scaling_rotation():
    z = np.load(os.path.join(G, "golden_cov3d.npz"))
    for key, mod in (("cov_mod1", 1.0), ("cov_mod037", 0.37)):
        ref = z[key]
        got = np.stack([oracle.cov3d(z["scales"][i], mod, z["quats"][i]) for i in range(ref.shape[0])])
        scale = np.abs(ref).max(axis=1, keepdims=True)
        assert (np.abs(got - ref) <= 2e-6 * scale + 1e-12).all()


def test_camera_matches_reference_camera():
    z = np.load(os.path.join(G, "golden_camera.npz"))
    for name in z["names"]:
        fx, fy = z[f"{name}_fov"]
        h, w = z[f"{name}_res"]
        cam = scenes.make_camera(z[f"{name}_R"], z[f"{name}_T"], float(fx), float(fy), int(h), int(w))
        np.testing.assert_allclose(cam.world_view_transform, z[f"{name}_wvt"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(cam.full_proj_transform, z[f"{name}_full"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(cam.camera_center, z[f"{name}_center"], rtol=0, atol=5e-6)
        np.testing.assert_allclose(scenes.projection_matrix(0.01, 100.0, float(fx), float(fy)).T, z[f"{name}_proj"],
                                   rtol=1e-6, atol=1e-7)


def test_projection_matches_reference_geom_transform_points():
    """The oracle's projection (forward.cu:196-200 restated: p_hom = P x, p_proj = p_hom / (p_hom.w + 1e-7), ndc2Pix) and its
    view-space depth against the reference's own Python projection, tools/gs_utils/graphics_utils.py:22-29
    `geom_transform_points`, on 256 points in front of each of the five golden cameras."""
    z = np.load(os.path.join(G, "golden_proj.npz"))
    c = np.load(os.path.join(G, "golden_camera.npz"))
    checked = 0
    for name in z["names"]:
        pts, ndc, view = z[f"{name}_points"], z[f"{name}_ndc"], z[f"{name}_view"]
        H, W = (int(v) for v in c[f"{name}_res"])
        fx, fy = (float(v) for v in c[f"{name}_fov"])
        P = pts.shape[0]
        rot = np.zeros((P, 4), np.float32)
        rot[:, 0] = 1
        f = oracle.forward(bg=np.zeros(3, np.float32), means3D=pts, opacities=np.full((P, 1), 0.5, np.float32),
                           viewmatrix=c[f"{name}_wvt"], projmatrix=c[f"{name}_full"], campos=c[f"{name}_center"],
                           tanfovx=np.tan(fx / 2), tanfovy=np.tan(fy / 2), H=H, W=W, colors_precomp=np.full((P, 3), 0.5, np.float32),
                           scales=np.full((P, 3), 0.02, np.float32), rotations=rot)
        vis = f.radii > 0
        assert vis.sum() > 0.9 * P          # (points sit inside 0.9 of the frustum, 0.3 .. 5 in front of the camera)
        want_x = ((ndc[:, 0].astype(np.float64) + 1.0) * W - 1.0) * 0.5        # ndc2Pix, auxiliary.h:41-44
        want_y = ((ndc[:, 1].astype(np.float64) + 1.0) * H - 1.0) * 0.5
        # float32 matmul of the reference vs the rasterizer's left-to-right sums: a few ulp of the homogeneous coordinates (measured: <= 2.5e-4 pixel)
        assert np.abs(f.means2D[vis, 0] - want_x[vis]).max() < 5e-4
        assert np.abs(f.means2D[vis, 1] - want_y[vis]).max() < 5e-4
        np.testing.assert_allclose(f.depths[vis], view[vis, 2], rtol=1e-6, atol=0)
        checked += int(vis.sum())
    assert checked > 1100


def test_inverse_sigmoid_round_trip():
    z = np.load(os.path.join(G, "golden_misc.npz"))
    x = z["x"].astype(np.float64)
    np.testing.assert_allclose(np.log(x / (1 - x)), z["inverse_sigmoid"], rtol=2e-6, atol=1e-6)


def test_gs_utils_helpers_match_the_reference():
    """fateavatar_amd.gs_utils vs the reference's RGB2SH / SH2RGB, get_expon_lr_func and getWorld2View2."""
    from fateavatar_amd import gs_utils
    z = np.load(os.path.join(G, "golden_misc.npz"))
    np.testing.assert_allclose(gs_utils.RGB2SH(z["rgb"]), z["RGB2SH"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gs_utils.SH2RGB(z["rgb"]), z["SH2RGB"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gs_utils.inverse_sigmoid(z["x"].astype(np.float64)), z["inverse_sigmoid"], rtol=2e-6, atol=1e-6)
    fa = gs_utils.get_expon_lr_func(1.6e-4, 1.6e-6, max_steps=30000)
    fb = gs_utils.get_expon_lr_func(1e-2, 1e-4, lr_delay_steps=1000, lr_delay_mult=0.01, max_steps=30000)
    fc = gs_utils.get_expon_lr_func(0.0, 0.0)
    for f, k in ((fa, "lr_a"), (fb, "lr_b"), (fc, "lr_c")):
        np.testing.assert_allclose([f(s) for s in z["lr_steps"]], z[k], rtol=1e-12, atol=0)
    assert fa(0) == 1.6e-4 and abs(fa(30000) - 1.6e-6) < 1e-18 and fa(-1) == 0.0
    np.testing.assert_array_equal(gs_utils.getWorld2View2(z["w2v_R"], z["w2v_t"]), z["w2v_plain"])
    np.testing.assert_array_equal(gs_utils.getWorld2View2(z["w2v_R"], z["w2v_t"], z["w2v_translate"], 1.7), z["w2v_moved"])
    np.testing.assert_allclose(scenes.world_to_view(z["w2v_R"], z["w2v_t"]), z["w2v_plain"], atol=2e-6)


def test_workload_shape_matches_survey():
    """SURVEY.md Appendix B measured the reference (run through a host shim) on config 2:
    351 non-empty 16x16 tiles, mean/max list 594/1570, all radii 4, 28.5 % covered pixels."""
    s = scenes.head_scene()
    f = oracle.forward(bg=s.bg, means3D=s.means3D, opacities=s.opacities, viewmatrix=s.camera.world_view_transform,
                       projmatrix=s.camera.full_proj_transform, campos=s.camera.camera_center,
                       tanfovx=s.camera.tanfovx, tanfovy=s.camera.tanfovy, H=512, W=512, shs=s.shs, sh_degree=3,
                       scales=s.scales, rotations=s.rotations)
    ln = f.ranges[:, 1] - f.ranges[:, 0]
    assert int((ln > 0).sum()) == 351
    assert int(ln.max()) == 1570
    assert abs(f.num_rendered - 208596) < 200
    assert set(np.unique(f.radii)) == {4}
    assert abs(float((f.final_T < 1).mean()) - 0.285) < 0.003


def test_knn_oracle_is_exact():
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(3000, 3)).astype(np.float32)
    got = oracle.knn_mean_dist2(pts)
    d = ((pts[:, None, :] - pts[None, :, :]) ** 2)
    d2 = (d[..., 0] + d[..., 1]) + d[..., 2]
    np.fill_diagonal(d2, np.inf)
    d2.sort(axis=1)
    ref = ((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / np.float32(3.0)
    np.testing.assert_array_equal(got, ref.astype(np.float32))


def test_knn_oracle_equals_float32_brute_force_on_awkward_point_sets():
    """The oracle's Morton-pruned search == plain float32 brute force with the reference's expressions, bit for bit, mean
    and nearest, on every point set the GPU k-NN tests use with P <= 6000: P = 1, 2 (inf) and 3 (FLT_MAX / 3), exact
    duplicates, a plane, a line, a lattice full of ties, far-offset, all-negative, clustered.  This pins the oracle as
    the reference for the point sets that are too large for brute force."""
    from tests import util
    sets = util.knn_point_sets()
    assert len(sets) >= 12
    for name, pts in sets.items():
        assert pts.dtype == np.float32 and pts.shape[0] <= 6000
        mean, nearest = oracle.knn_dist2(pts)
        want_mean, want_nearest = util.knn_brute_force(pts)
        np.testing.assert_array_equal(mean, want_mean, err_msg=name)
        np.testing.assert_array_equal(nearest, want_nearest, err_msg=name)
        np.testing.assert_array_equal(oracle.knn_mean_dist2(pts), want_mean, err_msg=name)
    assert np.all(np.isinf(oracle.knn_mean_dist2(sets["normal_2"]))) and np.isinf(oracle.knn_mean_dist2(sets["normal_1"])[0])
    assert abs(float(oracle.knn_mean_dist2(sets["normal_3"])[0]) / 1.1342e38 - 1) < 1e-3
    assert float(oracle.knn_dist2(sets["one_point_300_times"])[0].max()) == 0.0
