"""The host side of the three mesh-binding modes: what the one descriptor builder writes into fr_binding (and, for the Phong
mode, into the tail of fr_binding_phong), what every binding class says about its mode, and the one checked call into the
library.  No GPU: the builder reads only `.shape` and `.data_ptr()`, and the library is a stub."""
import ctypes as C

import pytest
import torch

from fateavatar_amd import _lib, binding
from fateavatar_amd.bound import FaceLocalBinding, MeshBinding, PhongBinding, _PhongView

V, F, N = 4, 2, 5
POINTERS = ("verts", "faces", "face_index", "bary", "face_scale_canonical", "offset", "rotation", "scaling", "local_xyz")


def _tensors():
    """Small DISTINCT tensors (no two share storage, so no two share a data_ptr)."""
    f32, i32 = torch.float32, torch.int32
    t = {"verts": torch.zeros(V, 3, dtype=f32), "faces": torch.zeros(F, 3, dtype=i32), "face_index": torch.zeros(N, dtype=i32),
         "bary": torch.zeros(N, 3, dtype=f32), "canon": torch.zeros(F, 1, dtype=f32), "offset": torch.zeros(N, 1, dtype=f32),
         "own3": torch.zeros(N, 3, dtype=f32), "rotation": torch.zeros(N, 4, dtype=f32), "scaling": torch.zeros(N, 3, dtype=f32),
         "vn": torch.zeros(V, 3, dtype=f32), "vq": torch.zeros(V, 4, dtype=f32), "ratio": torch.zeros(F, dtype=f32)}
    assert len({x.data_ptr() for x in t.values()}) == len(t)
    return t


def _build(mode, t, shell_len=0.05, resize_scale=True):
    """The descriptor of `mode` from the tensors `t`, as the package builds it."""
    if mode == "shell":
        return binding._describe(binding.SHELL, t["verts"], t["faces"], t["face_index"], t["offset"], t["rotation"], t["scaling"],
                                 bary=t["bary"], canon=t["canon"], shell_len=shell_len, resize_scale=resize_scale)
    if mode == "face_local":
        return binding._describe(binding.FACE_LOCAL, t["verts"], t["faces"], t["face_index"], t["own3"], t["rotation"], t["scaling"])
    return binding._describe(binding.PHONG, t["verts"], t["faces"], t["face_index"], t["own3"], t["rotation"], t["scaling"],
                             bary=t["bary"], frame=(t["vn"], t["vq"], t["ratio"]))


def _expect(b, t, mode, reads, shell_len, resize_scale):
    assert type(b) is _lib.fr_binding
    assert (b.N, b.V, b.F) == (N, V, F)
    assert b.mode == mode
    for field in POINTERS:
        got = getattr(b, field)
        if field in reads:
            assert got == t[reads[field]].data_ptr(), field
        else:
            assert got is None, field              # (a NULL c_void_p member reads back as None)
    assert b.shell_len == pytest.approx(shell_len, abs=0, rel=1e-7) and b.resize_scale == resize_scale
    assert {n for n, _ in _lib.fr_binding._fields_} == {"N", "V", "F", "mode", "shell_len", "resize_scale", *POINTERS}   # every field is covered


def test_shell_descriptor_fields():
    t = _tensors()
    b = _build("shell", t)
    _expect(b, t, _lib.FR_BIND_SHELL, {"verts": "verts", "faces": "faces", "face_index": "face_index", "bary": "bary",
                                       "face_scale_canonical": "canon", "offset": "offset", "rotation": "rotation",
                                       "scaling": "scaling"}, 0.05, 1)
    assert C.sizeof(b) == C.sizeof(_lib.fr_binding)                      # a plain fr_binding: no Phong tail behind it
    b = _build("shell", dict(t, canon=None), shell_len=0.25, resize_scale=False)      # (without resize_scale there is no canonical scale)
    assert b.face_scale_canonical is None and b.shell_len == 0.25 and b.resize_scale == 0


def test_face_local_descriptor_fields():
    t = _tensors()
    _expect(_build("face_local", t), t, _lib.FR_BIND_FACE_LOCAL,
            {"verts": "verts", "faces": "faces", "face_index": "face_index", "rotation": "rotation", "scaling": "scaling",
             "local_xyz": "own3"}, 0.0, 0)


def test_phong_descriptor_fields_and_tail():
    t = _tensors()
    b = _build("phong", t)
    _expect(b, t, _lib.FR_BIND_PHONG,
            {"verts": "verts", "faces": "faces", "face_index": "face_index", "bary": "bary", "rotation": "rotation",
             "scaling": "scaling", "local_xyz": "own3"}, 0.0, 0)
    # the mode's three arrays sit behind the fr_binding, in the memory the descriptor shares with its fr_binding_phong
    p = _lib.fr_binding_phong.from_address(C.addressof(b))
    assert (p.vert_normals, p.vert_quats, p.face_ratio) == (t["vn"].data_ptr(), t["vq"].data_ptr(), t["ratio"].data_ptr())
    assert p.base.N == N and p.base.local_xyz == t["own3"].data_ptr()


def test_binding_classes_name_their_mode():
    for cls, value, attr, grad in ((MeshBinding, _lib.FR_BIND_SHELL, "_offset", "d_offset"),
                                   (FaceLocalBinding, _lib.FR_BIND_FACE_LOCAL, "_xyz", "d_local_xyz"),
                                   (PhongBinding, _lib.FR_BIND_PHONG, "_uvd", "d_local_xyz"),
                                   (_PhongView, _lib.FR_BIND_PHONG, "_uvd", "d_local_xyz")):
        assert cls.mode.value == value and cls.mode.attr == attr and cls.mode.grad == grad
        assert "mode" not in cls._fields                                 # a class attribute, not a seventh field
    assert hasattr(_lib.fr_aux, "d_offset") and hasattr(_lib.fr_aux, "d_local_xyz")
    assert [m.active_sh for m in (binding.SHELL, binding.FACE_LOCAL, binding.PHONG)] == [False, True, False]
    assert [m.verts_grad for m in (binding.SHELL, binding.FACE_LOCAL, binding.PHONG)] == [True, True, False]
    assert [m.backward for m in (binding.SHELL, binding.FACE_LOCAL, binding.PHONG)] == \
        ["fr_bind_backward", "fr_bind_backward_local", "fr_bind_backward_phong"]
    with pytest.raises(AttributeError):
        binding.SHELL.value = 1                                          # immutable


class _StubLib:
    """Stands where the loaded library stands: one entry point that records its arguments and fails with code 3."""

    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def fr_stub_call(self, *args):
        self.calls.append(args)
        return self.rc

    def fr_last_error(self):
        return b"fr_stub_call: the stream is on fire"


class _NoDevice:
    def __init__(self, device):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_launch_appends_the_stream_and_raises_with_the_librarys_message(monkeypatch):
    import types
    monkeypatch.setattr(torch.cuda, "device", _NoDevice)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0x5EED))
    stub = _StubLib(_lib.FR_ERR_HIP)
    monkeypatch.setattr(_lib, "_lib", stub)
    with pytest.raises(RuntimeError, match=r"^fr_stub_call failed \(code 3\): fr_stub_call: the stream is on fire$"):
        _lib.launch("fr_stub_call", torch.device("cuda", 0), 7, None)
    assert stub.calls == [(7, None, 0x5EED)]                             # the current stream is the last argument
    ok = _StubLib(_lib.FR_OK)
    monkeypatch.setattr(_lib, "_lib", ok)
    assert _lib.launch("fr_stub_call", torch.device("cuda", 0), 1) is None and ok.calls == [(1, 0x5EED)]
