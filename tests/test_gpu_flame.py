"""-m gpu: the fused FLAME kernels (csrc/fr_flame.hip, fateavatar_amd/flame.py) on the device — forward and backward against the
float64 restatement of tests/flame_ref.py with a bound MEASURED on the float32 restatement, the same bits on every launch and
graph replay, the autograd op, and AvatarStep(flame=...) against the existing route (torch FLAME outside the step).

The bound (as tests/test_gpu_mlp.py): the float32 restatement on the CPU has a rel-L2 error e32 against float64 for each output;
the kernels may have at most FACTOR x e32 (another summation order) and never more than the project's gradient ceiling 1e-4.

The pose regimes (test_pose_regimes, test_trees_and_tables) are held to the float64 truth with the float32 run of the STABLE form
of the rotation as the yardstick (flame_ref.rotation_offset): below 3e-4 rad the reference's own float32 form loses up to four
digits of R - I (cos rounds to 1), sits at the ceiling itself and cannot bound a correct kernel.  Every comparison is also made
BLOCK BY BLOCK (_check_blocks): a whole-array rel-L2 lets one joint of d_pose or one row of d_delta_posedirs hide."""
import ctypes
import functools

import numpy as np
import pytest

from tests import flame_ref

pytestmark = pytest.mark.gpu

FACTOR, CEILING = 4.0, 1e-4
# (V, n_shape, n_exp): one vertex, an odd size below one skinning tile, the golden file's, a ragged size at the widest expression,
# FLAME's own vertex count, and one vertex past each grid cap (256 workgroups of 16 and of 64 vertices) at n_exp = 1
# and the sizes on either side of a lane group (16 lanes per vertex, 16 expression columns per sweep) and of a skinning tile (64)
SHAPES = [(1, 0, 1), (63, 0, 5), (300, 3, 7), (257, 2, 128), (5023, 100, 50), (4097, 0, 1), (16385, 0, 1),
          (16, 0, 15), (17, 0, 16), (64, 1, 17), (65, 0, 127)]
OUTPUTS = ("verts", "verts_orig", "pose_feature", "A", "d_delta_exp", "d_delta_posedirs", "d_delta_vertex", "d_expression", "d_pose")


ROW_FACTOR = 16             # tests/test_gpu_mono.py's: a block may miss float64 by this many times the float32 restatement's worst block
EPS = 2.0 ** -24
YARDSTICK_SHAPE = (4099, 3, 7)
FLAME_TREE = (-1, 0, 1, 1, 1)
SWEEP = (0.0, 1e-6, 5e-5, 1e-4, 2e-4, 2.4e-4, 3e-4, 1e-3, 3.1)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------ pose recipes, models, references
def _axes():
    import torch
    g = torch.Generator().manual_seed(77)
    return torch.nn.functional.normalize(torch.randn(5, 3, generator=g, dtype=torch.float64), dim=1)


def _pose(recipe, own):
    """A pose [15] (float32) by recipe: "randn" — the model's own 0.3 randn; ("theta", t) — five seeded unit axes x t; "rest" —
    joints 1, 3, 4 exactly zero, the model's own rotations at 0 and 2; "large" — the axes x 3.1, joint 2 x 6.2."""
    if recipe == "randn":
        return own.clone()
    if recipe == "rest":
        p = own.clone().view(5, 3)
        p[[1, 3, 4]] = 0.0
        return p.reshape(15)
    a = _axes()
    if recipe == "large":
        a = 3.1 * a
        a[2] = 2.0 * a[2]
        return a.reshape(15).float()
    assert recipe[0] == "theta"
    return (recipe[1] * a).reshape(15).float()


def _references(m):
    """The float64 truth (the reference's form), the float32 run of the reference's form and the float32 run of the stable form
    for the model dict `m`, each with `d_delta_exp` and `verts_orig`."""
    import torch
    out = {}
    for name, dtype, stable in (("r64", torch.float64, False), ("r32", torch.float32, False), ("r32s", torch.float32, True)):
        r = flame_ref.run(m, dtype, stable_rotation=stable)
        r["d_delta_exp"] = r.pop("d_delta_shapedirs")[:, :, m["n_shape"]:].contiguous()
        r["verts_orig"] = flame_ref.run(m, dtype, with_deltas=False, stable_rotation=stable)["verts"]
        out[name] = r
    return out


def _blocks(name, t, n_exp):
    """The array `name` as [blocks, -1], or None for an output that is held as a whole only."""
    if name in ("d_pose", "A", "pose_feature"):
        t = t[:, :3, :] if name == "A" else t
        return t.reshape(5 if name != "pose_feature" else 4, -1)
    if name == "d_delta_posedirs":
        return t.reshape(36, -1)
    if name == "d_delta_exp":
        return t.reshape(-1, n_exp).t()
    if name == "d_delta_vertex":
        return t.reshape(-1, 3)
    return None


BLOCKED = ("d_pose", "A", "pose_feature", "d_delta_posedirs", "d_delta_exp", "d_delta_vertex")


@functools.lru_cache(maxsize=None)
def _yardstick(recipe):
    """{output: the worst block (tests/test_gpu_mono._row_metric) of the float32 STABLE restatement against float64} at
    YARDSTICK_SHAPE with the pose recipe: on the CPU, computed once.  (A maximum over the few blocks of a small case is no
    yardstick — tests/test_gpu_mono.py.)"""
    import torch
    from tests.test_gpu_mono import _row_metric
    V, NS, NE = YARDSTICK_SHAPE
    m = flame_ref.random_model(V, NS, NE, seed=4099, dtype=torch.float32)
    m["pose"] = _pose(recipe, m["pose"])
    r = _references(m)
    return {n: float(_row_metric(_blocks(n, r["r32s"][n], NE), _blocks(n, r["r64"][n], NE)).max()) for n in BLOCKED}


def _check_blocks(got, r64, n_exp, recipe, label):
    """Every block of every blocked output within ROW_FACTOR x the recipe's yardstick, and never above CEILING."""
    import torch
    from tests.test_gpu_mono import _row_metric
    yard, missed = _yardstick(recipe), []
    for n in BLOCKED:
        ref = _blocks(n, r64[n], n_exp)
        if float(ref.abs().max()) == 0:         # (zero pose: the caller has held the kernel's values to exact zeros)
            assert recipe == ("theta", 0.0) and n in ("pose_feature", "d_delta_posedirs"), n
            continue
        m = _row_metric(_blocks(n, got[n].cpu(), n_exp), ref)
        worst, at = float(m.max()), int(m.argmax())
        print(f"{label} {n}: worst block {worst:.3e} (block {at} of {m.numel()}), yardstick {yard[n]:.3e}, "
              f"ratio {worst / yard[n]:.2f} of the {ROW_FACTOR} allowed")
        assert 0 < yard[n] <= 2e-6, (n, yard[n])
        if not (bool(torch.isfinite(m).all()) and worst <= min(ROW_FACTOR * yard[n], CEILING)):
            missed.append((label, n, at, worst, yard[n]))
    assert not missed, missed             # (after every output's line is printed)


def _check_stable(got, refs, label, zero_pose=False):
    """Every output against the float64 truth: at most FACTOR x the STABLE float32 run's error — and no less than FACTOR float32
    roundings, for an e32s that is accidentally nothing where another order of the joint sums alone moves a rounding — and
    never above CEILING.  `zero_pose`: pose_feature and d_delta_posedirs are exactly zero in float64, and here."""
    import torch
    r64, r32, r32s, missed = refs["r64"], refs["r32"], refs["r32s"], []
    for name in OUTPUTS:
        v, ref64 = got[name].cpu().reshape(-1), r64[name].reshape(-1)
        assert bool(torch.isfinite(v).all()), name
        if zero_pose and name in ("pose_feature", "d_delta_posedirs"):
            assert float(ref64.abs().max()) == 0 and int(v.count_nonzero()) == 0, name
            print(f"{label} {name}: exactly zero, as in float64")
            continue
        err, e32, e32s = _rel(v, ref64), _rel(r32[name].reshape(-1), ref64), _rel(r32s[name].reshape(-1), ref64)
        print(f"{label} {name}: kernel {err:.3e}  float32 reference form {e32:.3e}  float32 stable form {e32s:.3e}")
        assert float(ref64.abs().max()) > 0, name
        if not (err <= max(FACTOR * e32s, FACTOR * EPS) and err <= CEILING):
            missed.append((label, name, err, e32s))
    assert not missed, missed             # (after every output's line is printed)


@functools.lru_cache(maxsize=None)
def _case(V, NS, NE):
    """One model and its inputs on the CPU from a seed of the shape, with the float64 and the float32 restatement's results
    (computed once, shared, never modified)."""
    import torch
    m = flame_ref.random_model(V, NS, NE, seed=1000 * NE + 10 * NS + V, dtype=torch.float32)
    out = {}
    for name, dtype in (("r64", torch.float64), ("r32", torch.float32)):
        r = flame_ref.run(m, dtype)
        r["d_delta_exp"] = r.pop("d_delta_shapedirs")[:, :, NS:].contiguous()
        r["verts_orig"] = flame_ref.run(m, dtype, with_deltas=False)["verts"]
        out[name] = r
    return dict(m=m, **out)


def _mesh(m, dev):
    from fateavatar_amd.flame import FlameMesh
    fm = FlameMesh(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"], m["n_shape"],
                   m["n_exp"], device=dev)
    fm.load_state_dict({k: m[k] for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")})
    return fm


def _run(fm, m, dev, orig=True, poison=float("nan")):
    """One forward and one backward through the raw entry points into poisoned outputs: a dict of device tensors."""
    import torch
    full = lambda *s: torch.full(s, poison, device=dev)  # noqa: E731
    e, p, g = m["expression"].to(dev), m["pose"].to(dev), m["g"].to(dev)
    o = dict(verts=full(fm.V, 3), verts_orig=full(fm.V, 3) if orig else None, pose_feature=full(36), A=full(5, 4, 4),
             d_expression=full(fm.n_exp), d_pose=full(15))
    fm.flat_grad.fill_(poison)
    fm.forward_into(e, p, o["verts"], o["verts_orig"], o["pose_feature"], o["A"])
    fm.backward_from(g, e, p, o["d_expression"], o["d_pose"])
    o.update(d_delta_exp=fm.grad_delta_exp.clone(), d_delta_posedirs=fm.grad_delta_posedirs.clone(),
             d_delta_vertex=fm.grad_delta_vertex.clone())
    return o


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_float64(gpu_device, shape):
    import torch
    dev = gpu_device
    c = _case(*shape)
    m, r64, r32 = c["m"], c["r64"], c["r32"]
    fm = _mesh(m, dev)
    got = _run(fm, m, dev)
    torch.cuda.synchronize()
    assert int(fm.workspace_zeroed_part().count_nonzero()) == 0
    for name in OUTPUTS:
        v, ref64, ref32 = got[name].cpu().reshape(-1), r64[name].reshape(-1), r32[name].reshape(-1)
        assert bool(torch.isfinite(v).all()), name
        e32, err = _rel(ref32, ref64), _rel(v, ref64)
        print(f"V={shape[0]} NS={shape[1]} NE={shape[2]} {name}: kernel {err:.3e}  float32 restatement {e32:.3e}  "
              f"ratio {err / max(e32, 1e-300):.2f}")
        assert float(ref64.abs().max()) > 0
        assert err <= FACTOR * e32, (name, err, e32)
        assert err <= CEILING, (name, err)
    _check_blocks(got, r64, shape[2], "randn", f"V={shape[0]} NS={shape[1]} NE={shape[2]}")
    # without verts_orig, and with some outputs NULL: what the others receive are the same bits
    alone = _run(fm, m, dev, orig=False)
    for name in OUTPUTS:
        if name != "verts_orig":
            assert torch.equal(alone[name], got[name]), name
    e, p, g = m["expression"].to(dev), m["pose"].to(dev), m["g"].to(dev)
    d_pose = torch.full((15,), float("nan"), device=dev)
    fm.flat_grad.fill_(7.0)
    fm.backward_from(g, e, p, None, d_pose, deltas=False)
    assert torch.equal(d_pose, got["d_pose"]) and bool((fm.flat_grad == 7.0).all())
    d_e = torch.full((fm.n_exp,), float("nan"), device=dev)
    fm.backward_from(g, e, p, d_e, None)
    assert torch.equal(d_e, got["d_expression"]) and torch.equal(fm.grad_delta_posedirs, got["d_delta_posedirs"])
    torch.cuda.synchronize()
    assert int(fm.workspace_zeroed_part().count_nonzero()) == 0


def test_same_bits_on_every_launch_and_replay_and_outputs_are_overwritten(gpu_device):
    import torch
    from fateavatar_amd import _lib
    from fateavatar_amd.flame import FlameMesh
    dev = gpu_device
    c = _case(5023, 100, 50)
    m = c["m"]
    fm = _mesh(m, dev)
    first, second = _run(fm, m, dev, poison=float("nan")), _run(fm, m, dev, poison=-3.0e30)
    for name in OUTPUTS:
        assert torch.equal(first[name], second[name]), name
    # an eager call and a graph replay, into poisoned static outputs
    e, p, g = m["expression"].to(dev), m["pose"].to(dev), m["g"].to(dev)
    s = dict(verts=torch.empty(fm.V, 3, device=dev), verts_orig=torch.empty(fm.V, 3, device=dev), pose_feature=torch.empty(36, device=dev),
             A=torch.empty(5, 4, 4, device=dev), d_expression=torch.empty(50, device=dev), d_pose=torch.empty(15, device=dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fm.forward_into(e, p, s["verts"], s["verts_orig"], s["pose_feature"], s["A"])
        fm.backward_from(g, e, p, s["d_expression"], s["d_pose"])
    for _ in range(2):
        for t in s.values():
            t.fill_(float("nan"))
        fm.flat_grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for name, t in s.items():
            assert torch.equal(t, first[name]), name
        assert torch.equal(fm.grad_delta_exp, first["d_delta_exp"]) and torch.equal(fm.grad_delta_posedirs, first["d_delta_posedirs"])
        assert torch.equal(fm.grad_delta_vertex, first["d_delta_vertex"])
        assert int(fm.workspace_zeroed_part().count_nonzero()) == 0
    # stored, not accumulated: g = 0 gives exact zeros over the poison
    zero = _run(fm, m | {"g": torch.zeros_like(m["g"])}, dev, poison=5.0)
    for name in ("d_delta_exp", "d_delta_posedirs", "d_delta_vertex", "d_expression", "d_pose"):
        assert int(zero[name].count_nonzero()) == 0, name
    # V = 0 launches nothing; sizes outside the limits are refused by the entry points themselves
    empty = FlameMesh(torch.zeros(0, 3), torch.zeros(0, 3, 4), torch.zeros(36, 0), torch.zeros(5, 0), [-1, 0, 1, 1, 1], torch.zeros(0, 5),
                      1, 3, device=dev)
    d_e = torch.full((3,), float("nan"), device=dev)
    empty.forward_into(torch.zeros(3, device=dev), torch.zeros(15, device=dev), torch.empty(0, 3, device=dev))
    empty.backward_from(torch.empty(0, 3, device=dev), torch.zeros(3, device=dev), torch.zeros(15, device=dev), d_e)
    assert int(d_e.count_nonzero()) == 0
    d = fm._desc(e, p)
    d.NE = _lib.FR_FLAME_MAX_E + 1
    with pytest.raises(RuntimeError, match="FR_FLAME_MAX_E"):
        _lib.launch("fr_flame_forward", dev, ctypes.byref(d), s["verts"].data_ptr(), None, None, None, fm._workspace.data_ptr())
    d.NE, d.pose = 50, None
    with pytest.raises(RuntimeError, match="null parents, expression or pose"):
        _lib.launch("fr_flame_backward", dev, ctypes.byref(d), g.data_ptr(), None, None, None, None, None, fm._workspace.data_ptr())


def test_autograd_op_hands_out_the_same_gradients(gpu_device):
    import torch
    dev = gpu_device
    c = _case(300, 3, 7)
    m = c["m"]
    fm = _mesh(m, dev)
    raw = _run(fm, m, dev)
    e, p = m["expression"].to(dev).requires_grad_(True), m["pose"].to(dev).requires_grad_(True)
    verts, phi, A = fm(e, p)
    assert verts.requires_grad and not phi.requires_grad and not A.requires_grad
    assert torch.equal(verts.detach(), raw["verts"]) and torch.equal(phi, raw["pose_feature"]) and torch.equal(A, raw["A"])
    # another frame goes through the same FlameMesh before the backward: the op restores its own frame's state
    fm(torch.zeros_like(e), torch.zeros_like(p))
    verts.backward(m["g"].to(dev))
    assert torch.equal(fm.flat.grad, fm.flat_grad) and fm.flat.grad.data_ptr() != fm.flat_grad.data_ptr()
    assert torch.equal(fm.grad_delta_exp, raw["d_delta_exp"]) and torch.equal(fm.grad_delta_vertex, raw["d_delta_vertex"])
    assert torch.equal(e.grad, raw["d_expression"]) and torch.equal(p.grad, raw["d_pose"])
    assert _rel(p.grad.cpu(), c["r64"]["d_pose"]) <= CEILING
    with pytest.raises(ValueError, match=r"contiguous \[7\]"):
        fm(torch.zeros(6, device=dev), p)
    with pytest.raises(TypeError, match="float32"):
        fm(e.detach(), torch.zeros(15, device=dev, dtype=torch.float64))


# ------------------------------------------------------------------ pose regimes, joint trees, tables
@functools.lru_cache(maxsize=None)
def _regime(recipe, parents=FLAME_TREE, tables="random"):
    """The (300, 3, 7) model with the pose of `recipe`, the joint tree `parents` and `tables`: "random" — flame_ref.random_model's;
    "onehot" — every vertex skinned to ONE joint (FLAME's own weights hold exact 0 and 1) and a regressor of four non-zeros per
    joint; "onehot_no_4" — the same with no vertex on joint 4.  With its references, computed once."""
    import torch
    m = flame_ref.random_model(300, 3, 7, seed=5, dtype=torch.float32)
    m["pose"] = _pose(recipe, m["pose"])
    m["parents"] = torch.tensor(parents)
    if tables != "random":
        g = torch.Generator().manual_seed(9)
        used = 5 if tables == "onehot" else 4
        joint = torch.randint(0, used, (300,), generator=g)
        joint[:used] = torch.arange(used)                       # every joint in use owns a vertex
        m["lbs_weights"] = torch.nn.functional.one_hot(joint, 5).float()
        Jr = torch.zeros(5, 300, dtype=torch.float64)
        for j in range(5):
            w = torch.rand(4, generator=g, dtype=torch.float64) + 0.1
            Jr[j, torch.randperm(300, generator=g)[:4]] = w / w.sum()
        m["J_regressor"] = Jr.float()
        assert int((m["lbs_weights"][:, 4] != 0).sum()) == (0 if tables == "onehot_no_4" else int((joint == 4).sum()))
        assert bool(((m["J_regressor"] != 0).sum(1) == 4).all())
    return dict(m=m, **_references(m))


REGIMES = [("theta", t) for t in SWEEP] + ["rest"]


@pytest.mark.parametrize("recipe", REGIMES, ids=lambda r: r if isinstance(r, str) else f"theta={r[1]:g}")
def test_pose_regimes_against_float64(gpu_device, recipe):
    """Five seeded unit axes x theta from exact zero through the band where float32's cos rounds to 1 (below 2.4e-4 rad) to 3.1,
    and a pose with three joints exactly at rest: what real tracks hold (neck and eyes at zero, rotations of 1e-5 .. 1e-3).
    The truth is float64; the bound is the float32 run of the stable form (see the module's docstring)."""
    import torch
    c = _regime(recipe)
    fm = _mesh(c["m"], gpu_device)
    got = _run(fm, c["m"], gpu_device)
    torch.cuda.synchronize()
    assert int(fm.workspace_zeroed_part().count_nonzero()) == 0
    label = recipe if isinstance(recipe, str) else f"theta={recipe[1]:g}"
    _check_stable(got, c, label, zero_pose=recipe == ("theta", 0.0))
    _check_blocks(got, c["r64"], 7, recipe, label)


TREES = {"chain": (-1, 0, 1, 2, 3), "star": (-1, 0, 0, 0, 0), "mixed": (-1, 0, 0, 1, 2)}


@pytest.mark.parametrize("which", list(TREES) + ["onehot", "onehot_no_4"])
def test_trees_and_tables_against_float64(gpu_device, which):
    """Joint trees other than FLAME's own (a chain four deep, a star, a mixed tree: fl_parents / fl_chain_forward / _backward are
    written for any parents[i] < i) and tables with exact zeros and ones, at rotations of a few tenths of a radian."""
    import torch
    c = _regime("randn", TREES.get(which, FLAME_TREE), "random" if which in TREES else which)
    fm = _mesh(c["m"], gpu_device)
    assert fm.parents.tolist() == list(TREES.get(which, FLAME_TREE))
    got = _run(fm, c["m"], gpu_device)
    torch.cuda.synchronize()
    _check_stable(got, c, which)
    _check_blocks(got, c["r64"], 7, "randn", which)
    # (the tree matters: FLAME's own gives another mesh)
    if which in TREES:
        assert _rel(c["r64"]["verts"], _regime("randn")["r64"]["verts"]) > 1e-3


# ------------------------------------------------------------------ NULL delta inputs (include/fr_rasterizer.h: "NULL: zeros")
def _raw(fm, m, dev, null=()):
    """One forward and backward through the C entry points with the descriptor's delta pointers named in `null` set to NULL,
    into poisoned outputs (the gradients of all three deltas are still asked for)."""
    import torch
    from fateavatar_amd import _lib
    full = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    e, p, g = m["expression"].to(dev), m["pose"].to(dev), m["g"].to(dev)
    d = fm._desc(e, p)
    for k in null:
        assert getattr(d, k) is not None
        setattr(d, k, None)
        assert getattr(d, k) is None
    o = dict(verts=full(fm.V, 3), verts_orig=full(fm.V, 3), pose_feature=full(36), A=full(5, 4, 4), d_expression=full(fm.n_exp),
             d_pose=full(15))
    fm.flat_grad.fill_(float("nan"))
    ws = fm._workspace.data_ptr()
    _lib.launch("fr_flame_forward", dev, ctypes.byref(d), o["verts"].data_ptr(), o["verts_orig"].data_ptr(), o["pose_feature"].data_ptr(),
                o["A"].data_ptr(), ws)
    _lib.launch("fr_flame_backward", dev, ctypes.byref(d), g.data_ptr(), fm.grad_delta_exp.data_ptr(), fm.grad_delta_posedirs.data_ptr(),
                fm.grad_delta_vertex.data_ptr(), o["d_expression"].data_ptr(), o["d_pose"].data_ptr(), ws)
    o.update(d_delta_exp=fm.grad_delta_exp.clone(), d_delta_posedirs=fm.grad_delta_posedirs.clone(),
             d_delta_vertex=fm.grad_delta_vertex.clone())
    torch.cuda.synchronize()
    assert int(fm.workspace_zeroed_part().count_nonzero()) == 0
    return o


def test_null_delta_inputs_are_zeros_bit_for_bit(gpu_device):
    import torch
    dev = gpu_device
    m = _case(300, 3, 7)["m"]
    fm = _mesh(m, dev)
    with_deltas = _raw(fm, m, dev)
    assert torch.equal(with_deltas["verts"], _run(fm, m, dev)["verts"])
    # ---- all three NULL: the plain mesh, and the bits of a FlameMesh whose flat buffer is all zeros
    zeros = _mesh(m, dev)
    with torch.no_grad():
        zeros.flat.zero_()
    want = _raw(zeros, m, dev)
    got = _raw(fm, m, dev, null=("delta_exp", "delta_posedirs", "delta_vertex"))
    assert torch.equal(got["verts"], with_deltas["verts_orig"]) and torch.equal(got["verts_orig"], with_deltas["verts_orig"])
    assert not torch.equal(got["verts"], with_deltas["verts"])
    for name in OUTPUTS:
        assert bool(torch.isfinite(got[name]).all()) and torch.equal(got[name], want[name]), name
    # ---- each single NULL: the bits of that delta set to zeros
    for k, view in (("delta_exp", "delta_exp"), ("delta_posedirs", "delta_posedirs"), ("delta_vertex", "delta_vertex")):
        one = _mesh(m, dev)
        with torch.no_grad():
            getattr(one, view).zero_()
        assert int(one.flat.count_nonzero()) > 0
        want, got = _raw(one, m, dev), _raw(fm, m, dev, null=(k,))
        for name in OUTPUTS:
            assert torch.equal(got[name], want[name]), (k, name)
        assert not torch.equal(got["verts"], with_deltas["verts"]), k


# ------------------------------------------------------------------ the step
P_STEP, RES_STEP, NS_STEP, NE_STEP = 2000, 128, 4, 10


@functools.lru_cache(maxsize=None)
def _step_setup(n_frames):
    """The head template centred on the origin (as FLAME's own template is), a synthetic FLAME over it with small non-zero
    deltas, `n_frames` frames of (camera, expression, pose) and target images of a hidden avatar on the float64-posed mesh."""
    import torch
    from fateavatar_amd import flame, mesh_sampling, scenes
    from fateavatar_amd.avatar import AvatarGaussians, AvatarStep, _BoundFrame
    from fateavatar_amd.binding import bind_gaussians
    from fateavatar_amd.knn import init_scale_by_knn
    from fateavatar_amd.model import TorchCamera
    from fateavatar_amd.render import render
    dev = torch.device("cuda:0")
    verts, faces, _ = scenes.head_geometry()
    verts = (verts - verts.mean(0)).astype(np.float32)
    rng = np.random.default_rng(4)
    fi, bc = mesh_sampling.random_sampling_barycoords(P_STEP, verts, faces, rng)
    pts = (verts[faces[fi]] * bc[:, :, None]).sum(1).astype(np.float32)
    scale_init = float(init_scale_by_knn(torch.from_numpy(pts).to(dev))[2])
    make = lambda: AvatarGaussians(fi, bc, scale_init, dev)  # noqa: E731
    g = torch.Generator().manual_seed(12)
    V, L = len(verts), NS_STEP + NE_STEP
    deltas = dict(delta_shapedirs=5e-4 * torch.randn(V, 3, L, generator=g), delta_posedirs=5e-4 * torch.randn(36, 3 * V, generator=g),
                  delta_vertex=2e-3 * torch.randn(V, 3, generator=g))

    def model():
        fm = flame.synthetic_flame(verts, seed=1, n_shape=NS_STEP, n_exp=NE_STEP, device=dev)
        fm.load_state_dict(deltas)
        return fm
    fm = model()
    frames = [flame.FlameFrame((0.5 * torch.randn(NE_STEP, generator=g)).to(dev), (0.1 * torch.randn(15, generator=g)).to(dev))
              for _ in range(n_frames)]
    cams = []
    for _ in range(n_frames):
        eye = np.array([0.25 * rng.uniform(-1, 1), 0.15 * rng.uniform(-1, 1), 0.8 + 0.1 * rng.uniform(-1, 1)], np.float32)
        cams.append(TorchCamera(scenes.look_at_camera(eye, np.zeros(3), (0, 1, 0), 0.5, 0.5, RES_STEP, RES_STEP), dev))
    faces_t, canon, bg = torch.from_numpy(faces).to(dev), torch.from_numpy(verts).to(dev), torch.ones(3, device=dev)
    gt = make()
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(gt.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
    ref = AvatarStep(gt, faces_t, canon, cams[0].clone(), bg, use_graph=False)
    gts = []
    with torch.no_grad():
        for f in range(n_frames):
            shown = _posed(fm, frames[f], torch.float64)[0].float().contiguous()
            xyz, rot, scl = bind_gaussians(shown, ref.faces, gt.face_index, gt.bary_coords, ref.face_scale_canonical, gt._offset,
                                           gt._rotation, gt._scaling, ref.shell_len, True)
            gts.append(render(cams[f], _BoundFrame(xyz, gt, rot, scl, None), bg)["render"].clone())
    return dict(dev=dev, make=make, model=model, frames=frames, cams=cams, faces=faces_t, canon=canon, bg=bg, gts=gts, deltas=deltas)


def _posed(fm, frame, dtype, leaves=None):
    """(verts, verts_orig) of the torch restatement on the FlameMesh's own tables, on its device, in `dtype`; `leaves`: the
    (delta_shapedirs, delta_posedirs, delta_vertex, expression, pose) to differentiate through, else the mesh's values."""
    c = lambda t: t.detach().to(dtype)  # noqa: E731
    sd = fm.state_dict()
    dS, dP, dV, e, p = leaves if leaves is not None else (c(sd["delta_shapedirs"]), c(sd["delta_posedirs"]), c(sd["delta_vertex"]),
                                                          c(frame.expression), c(frame.pose))
    tables = (c(fm.v_template), c(fm.shapedirs), c(fm.posedirs), c(fm.J_regressor), fm.parents.cpu(), c(fm.lbs_weights), fm.n_shape)
    verts = flame_ref.lbs(e, p, *tables, dS, dP, dV)[0]
    orig = flame_ref.lbs(e.detach(), p.detach(), *tables)[0]
    return verts, orig


def test_one_fused_step_matches_the_torch_route(gpu_device):
    """ONE eager step from identical state: the existing route (float32 torch FLAME on the device -> AvatarStep(mesh_terms) ->
    posed.backward(step.d_verts)) against AvatarStep(flame=..., mesh_terms=...)."""
    import torch
    from fateavatar_amd.avatar import AvatarBatchStep, AvatarStep
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    S = _step_setup(6)
    dev, f = S["dev"], 1
    frame, cam, gt = S["frames"][f], S["cams"][f], S["gts"][f]
    # ---- the existing route
    fm_t = S["model"]()
    sd = fm_t.state_dict()
    leaves = [sd[k].clone().requires_grad_(True) for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")] + \
             [frame.expression.clone().requires_grad_(True), frame.pose.clone().requires_grad_(True)]
    posed, orig = _posed(fm_t, frame, torch.float32, leaves)
    st_t = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False, mesh_terms=REFERENCE_MESH_TERMS)
    st_t.step(cam, posed, gt, verts_orig=orig.detach())
    posed.backward(st_t.d_verts)
    assert int(leaves[0].grad[:, :, :NS_STEP].count_nonzero()) == 0
    want_flat = torch.cat([leaves[0].grad[:, :, NS_STEP:].reshape(-1), leaves[1].grad.reshape(-1), leaves[2].grad.reshape(-1)])
    # ---- the fused step
    fm = S["model"]()
    w0 = fm.flat.detach().clone()
    st_f = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False, mesh_terms=REFERENCE_MESH_TERMS,
                      flame=fm)
    assert st_f.vertex_grad
    with pytest.raises(ValueError, match="FlameFrame"):
        st_f.step(cam, posed.detach(), gt)                                   # a vertex tensor
    with pytest.raises(ValueError, match="FlameFrame"):
        st_f.step(cam, frame, gt, verts_orig=orig.detach())
    assert st_f.host_steps == 0
    with pytest.raises(NotImplementedError, match="flame"):
        AvatarBatchStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], views_per_step=2, flame=fm)
    loss = st_f.step(cam, frame, gt)
    torch.cuda.synchronize()
    # (the two posed meshes differ by float32 rounding, and the loss is a mean of smooth terms of them)
    assert abs(float(loss) - float(st_t.loss)) <= 1e-4 * abs(float(st_t.loss))
    assert _rel(st_f.verts, posed.detach()) <= 1e-6 and _rel(st_f.verts_orig, orig.detach()) <= 1e-6
    for name, got, ref in (("d_verts", st_f.d_verts, st_t.d_verts), ("flat_grad", fm.flat_grad, want_flat),
                           ("d_expression", st_f.d_expression, leaves[3].grad), ("d_pose", st_f.d_pose, leaves[4].grad)):
        err = _rel(got, ref)
        print(f"fused step against the torch route, {name}: rel-L2 {err:.3e}")
        assert float(ref.abs().max()) > 0 and err <= CEILING, (name, err)
    # the wiring of the second Adam: the deltas are what torch.optim.Adam makes of the kernel's OWN gradient, group by group
    a, b, _ = fm.counts
    parts = [w0[:a].clone().requires_grad_(True), w0[a:a + b].clone().requires_grad_(True), w0[a + b:].clone().requires_grad_(True)]
    for q, gq in zip(parts, (fm.flat_grad[:a], fm.flat_grad[a:a + b], fm.flat_grad[a + b:])):
        q.grad = gq.clone()
    lrs = (1e-5, 1e-5, 1e-4)
    torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(parts, lrs)], lr=0.0).step()
    want = torch.cat([q.detach() for q in parts])
    rate = torch.cat([torch.full_like(q.detach(), lr) for q, lr in zip(parts, lrs)])
    diff = (fm.flat.detach() - want).abs()
    assert float((fm.flat.detach() - w0).abs().max()) > 0.5 * 1e-4
    assert bool((diff <= 1e-6 * want.abs() + 1e-6 * rate).all()), float(diff.max())
    assert st_f.flame_adam.step_count == 1 == st_f.adam.step_count


def test_fused_step_trains_as_one_graph_and_round_trips_its_checkpoint(gpu_device):
    import torch
    from fateavatar_amd.avatar import AvatarStep
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    from tests import util
    n_frames, steps = 6, 30
    S = _step_setup(n_frames)
    dev = S["dev"]
    fm, pc = S["model"](), S["make"]()
    w0 = fm.flat.detach().clone()
    st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=True, mesh_terms=REFERENCE_MESH_TERMS, flame=fm)
    losses = []
    for it in range(steps):
        f = it % n_frames
        losses.append(float(st.step(S["cams"][f], S["frames"][f], S["gts"][f])))
    torch.cuda.synchronize()
    st.check()
    assert st._graph is not None and st.overflows == 0
    print("loss, first and last 6 steps:", np.mean(losses[:6]), np.mean(losses[-6:]))
    assert np.mean(losses[-6:]) < np.mean(losses[:6]), (losses[:6], losses[-6:])
    applied = st.host_steps - st.skipped_steps
    assert st.host_steps == steps and st.flame_adam.step_count == applied == st.adam.step_count
    assert float((fm.flat.detach() - w0).abs().max()) > 0
    assert tuple(st.d_expression.shape) == (NE_STEP,) and float(st.d_expression.abs().max()) > 0 and float(st.d_pose.abs().max()) > 0
    assert torch.equal(fm.delta_shape_columns, S["deltas"]["delta_shapedirs"][:, :, :NS_STEP].to(dev))     # never trained
    # ---- the checkpoint carries the deltas in the reference's shapes and loads them back
    sd = st.state_dict()
    V = fm.V
    assert {k: tuple(sd["model"][k].shape) for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")} == \
        {"delta_shapedirs": (V, 3, NS_STEP + NE_STEP), "delta_posedirs": (36, 3 * V), "delta_vertex": (V, 3)}
    sd["model"]["flame.shapedirs"] = torch.zeros(2)                 # (something of the reference's that stays ignored)
    fm2 = S["model"]()
    st2 = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False,
                     mesh_terms=REFERENCE_MESH_TERMS, flame=fm2)
    assert st2.load_state_dict(sd) == ["flame.shapedirs"]
    assert torch.equal(fm2.flat, fm.flat) and torch.equal(st2.pc.flat, pc.flat)
    assert st2.flame_adam.step_count == applied == st2.adam.step_count
    before = fm.flat.detach().clone()
    for s in (st, st2):
        s.step(S["cams"][2], S["frames"][2], S["gts"][2])
    torch.cuda.synchronize()
    # the restored step goes on with the same update (the frame's gradients carry the rasterizer's float-atomic noise)
    assert _rel(fm2.flat.detach() - before, fm.flat.detach() - before) < 1e-2 and float((fm.flat.detach() - before).abs().max()) > 0
    util.assert_same_trajectory(st2.pc.flat, pc.flat, "checkpoint round trip", tight=2e-3)
    assert st2.flame_adam.step_count == applied + 1
    # without a FLAME model the same checkpoint loads as before: the deltas come back as ignored keys
    plain = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False)
    assert plain.load_state_dict(sd) == sorted(["delta_shapedirs", "delta_posedirs", "delta_vertex", "flame.shapedirs"])
