"""Generate tests/golden/golden_phongsurf.npz from the reference's importable Python.

Runs ONLY in the build container (needs /root/reference); the fixture it writes is plain data (inputs + recorded results) and
is committed.  No test imports this file.  Run as

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_phongsurf_golden.py

What is pinned: PhongSurfacePy3d.solve_delta_vwd (submodules/simple_phongsurf/simple_phongsurf/phongsurf_py3d.py:256-309) with
retrieve_vertices / retrieve_normals (:312-327), unmodified, on the CPU.  The module's two imports that do not exist here
(pytorch3d.ops, the compiled `triwalk`) are replaced by empty stand-in modules, and the object is made without __init__ (which
would construct the compiled walk): V, F, N are registered as its __init__ registers them.  The C++ walk cannot be built here
(the bundled Eigen lacks Eigen/Core), so nothing of it is recorded.

Every case is on the head template (fateavatar_amd/data/head_template_geom.npz) with area-weighted vertex normals; the points
come from `sample_bary_on_triangles` with a seed; a query is the point of the surface + N(0, sigma).  Per case:
  <case>_fidx [n] int32, <case>_uv [n,2], <case>_query [n,3]   the inputs
  <case>_delta [n,3] float32      solve_delta_vwd's result
  <case>_iters                    its iteration count: torch.optim.Adam.step calls counted around the unmodified function
  <case>_delta64 [n,3] float64, <case>_iters64   the same function on .double() buffers with torch's default dtype float64 (the
                                  function creates `delta` with the default dtype)
  <case>_inner                    inner_loop
Cases: `n96_s4` (the FIRST 96 points of `n3000_s4`, alone: the loss is a mean over all 3 n numbers, so they move differently),
`n3000_s05`, `n3000_s4`, `n3000_s20` (one set of points; sigma 0.5 / 4 / 20 mm — 20 mm is the regime of a split),
`n65_surface` (queries exactly on the surface: one iteration, delta 0), `n8_long` (inner_loop 500, sigma 0.5 mm).
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "submodules", "simple_phongsurf"))
sys.path.insert(0, ROOT)

for name in ("pytorch3d", "pytorch3d.ops", "simple_phongsurf.triwalk"):
    sys.modules.setdefault(name, types.ModuleType(name))

from simple_phongsurf.phongsurf_py3d import PhongSurfacePy3d  # noqa: E402

from fateavatar_amd.splatting import sample_bary_on_triangles  # noqa: E402


def vertex_normals(verts, faces):
    t = verts[faces]
    fn = torch.linalg.cross(t[:, 2] - t[:, 1], t[:, 0] - t[:, 1], dim=1)
    vn = torch.zeros_like(verts)
    for k in range(3):
        vn.index_add_(0, faces[:, k], fn)
    return torch.nn.functional.normalize(vn, eps=1e-6, dim=1)


def surface(V, F, N, inner_loop, dtype):
    s = PhongSurfacePy3d.__new__(PhongSurfacePy3d)
    torch.nn.Module.__init__(s)
    s.register_buffer("V", V.to(dtype))
    s.register_buffer("F", F.long())
    s.register_buffer("N", N.to(dtype))
    s.inner_loop, s.max_dist, s.method, s.verbose = inner_loop, torch.inf, "uvd", False
    return s


def counted(fn, *args):
    calls = [0]
    step = torch.optim.Adam.step

    def counting(self, *a, **k):
        calls[0] += 1
        return step(self, *a, **k)

    torch.optim.Adam.step = counting
    try:
        with torch.enable_grad():
            out = fn(*args)
    finally:
        torch.optim.Adam.step = step
    return out, calls[0]


def main():
    g = np.load(os.path.join(ROOT, "fateavatar_amd", "data", "head_template_geom.npz"))
    V, F = torch.from_numpy(g["verts"]).float(), torch.from_numpy(g["faces"]).long()
    N = vertex_normals(V, F)
    out, notes = {}, []

    def case(name, fidx, bary, sigma, inner_loop, seed, query=None):
        uv = bary[:, :2].contiguous()
        s32 = surface(V, F, N, inner_loop, torch.float32)
        if query is None:
            query = s32.retrieve_vertices(fidx, uv)
        if sigma > 0:
            query = query + torch.randn(query.shape, generator=torch.Generator().manual_seed(seed)) * sigma
        d32, it32 = counted(s32.solve_delta_vwd, query, fidx, uv)
        torch.set_default_dtype(torch.float64)
        try:
            d64, it64 = counted(surface(V, F, N, inner_loop, torch.float64).solve_delta_vwd, query.double(), fidx, uv.double())
        finally:
            torch.set_default_dtype(torch.float32)
        assert d32.dtype == torch.float32 and d64.dtype == torch.float64
        out.update({f"{name}_fidx": fidx.numpy().astype(np.int32), f"{name}_uv": uv.numpy(), f"{name}_query": query.numpy(),
                    f"{name}_delta": d32.numpy(), f"{name}_iters": np.int32(it32), f"{name}_delta64": d64.numpy(),
                    f"{name}_iters64": np.int32(it64), f"{name}_inner": np.int32(inner_loop)})
        diff = float((d32.double() - d64).abs().max())
        print(f"{name}: n {fidx.numel()} sigma {sigma} iterations {it32} (float64 {it64}) max|delta32 - delta64| {diff:.3e} "
              f"max|delta_uv| {float(d32[:, :2].abs().max()):.3f}")
        return query

    fidx, bary = sample_bary_on_triangles(int(F.shape[0]), 3000, torch.Generator().manual_seed(20))
    q4 = case("n3000_s4", fidx, bary, 0.004, 50, 104)
    case("n96_s4", fidx[:96], bary[:96], 0.0, 50, 0, query=q4[:96].clone())   # the same 96 points and queries, alone
    case("n3000_s05", fidx, bary, 0.0005, 50, 105)
    case("n3000_s20", fidx, bary, 0.020, 50, 120)
    f65, b65 = sample_bary_on_triangles(int(F.shape[0]), 65, torch.Generator().manual_seed(65))
    case("n65_surface", f65, b65, 0.0, 50, 0)
    f8, b8 = sample_bary_on_triangles(int(F.shape[0]), 8, torch.Generator().manual_seed(8))
    case("n8_long", f8, b8, 0.0005, 500, 108)
    it = int(out["n8_long_iters"])
    notes.append(f"n8_long stopped after {it} of 500 iterations: "
                 + ("an intermediate global stop is pinned" if 1 < it < 500 else "NO intermediate global stop is pinned by this case"))
    out["notes"] = np.array(notes)
    print(notes[0])
    path = os.path.join(OUT, "golden_phongsurf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
