"""OBJ reader (pytorch3d.io.load_obj stand-in for the head template)."""
import numpy as np

from fateavatar_amd import scenes
from fateavatar_amd.obj import load_obj


def test_small_obj_with_quads_uvs_and_relative_indices(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# comment\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\n"
                 "f 1/1/1 2/2/1 3/3/1 4/4/1\nf -4//1 -3//1 -2//1\nf 1 3 4\n")
    m = load_obj(str(p))
    assert m["verts"].shape == (4, 3) and m["verts_uvs"].shape == (4, 2)
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3]]
    assert m["faces_uvs"].tolist() == [[0, 1, 2], [0, 2, 3], [-1, -1, -1], [-1, -1, -1]]


def test_head_template_round_trips_through_the_obj_reader(tmp_path):
    """The head template as an exporter lays it out (comment header, mtllib / o / usemtl / s statements, one vn per face,
    v/vt/vn corners), written from the geometry fixture the repository ships: the reader gives back exactly the fixture's
    vertices, triangles, UV coordinates and per-corner UV indices, which are what scenes.head_geometry() serves."""
    verts, faces, kind = scenes.head_geometry()
    assert kind == "head_template" and verts.shape == (5023, 3) and faces.shape == (10006, 3)
    z = np.load(scenes.HEAD_GEOM)
    vt, ft = z["verts_uvs"], z["faces_uvs"]
    tri = verts[faces].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    lines = ["# head template, written from fateavatar_amd/data/head_template_geom.npz", "mtllib head.mtl", "o head_template"]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in verts.tolist()]                  # (%.9g: float32 round-trips exactly)
    lines += ["vt %.9g %.9g" % tuple(t) for t in vt.tolist()]
    lines += ["vn %.4f %.4f %.4f" % tuple(x) for x in n.tolist()]
    lines += ["usemtl material_1", "s off"]
    lines += ["f " + " ".join(f"{a + 1}/{b + 1}/{k + 1}" for a, b in zip(fv, fu))
              for k, (fv, fu) in enumerate(zip(faces.tolist(), ft.tolist()))]
    p = tmp_path / "head_template.obj"
    p.write_text("\n".join(lines) + "\n")
    m = load_obj(str(p))
    assert np.array_equal(m["verts"], verts) and np.array_equal(m["faces"], faces)
    assert np.array_equal(m["verts_uvs"], vt) and np.array_equal(m["faces_uvs"], ft)
    assert m["verts_uvs"].shape[1] == 2 and m["faces_uvs"].shape == faces.shape and m["faces_uvs"].min() >= 0
