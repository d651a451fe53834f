"""The step helpers around the rasterizer: fused L1 loss + gradient, one-launch input copies."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(3, 512, 512), (3, 37, 53), (1, 1, 3), (3, 1024, 1024)])
def test_l1_loss_and_grad_matches_autograd(gpu_device, shape):
    """reference: nn.L1Loss(reduction='mean') + backward (model/loss.py:92).  Loss to 1e-6 relative (different summation
    order), gradient exactly sign(img - gt) / n — including 0 where the two agree."""
    from fateavatar_amd.loss import l1_loss_and_grad
    g = torch.Generator(device="cpu").manual_seed(sum(shape))
    img = torch.rand(shape, generator=g).to(gpu_device)
    gt = torch.rand(shape, generator=g).to(gpu_device)
    gt.view(-1)[::7] = img.view(-1)[::7]          # exact ties: sign(0) = 0
    ref_in = img.clone().requires_grad_(True)
    ref = torch.nn.functional.l1_loss(ref_in, gt)
    ref.backward()
    for _ in range(3):                             # the workspace must come back zeroed: repeat
        loss, grad = l1_loss_and_grad(img, gt)
        torch.cuda.synchronize()
        assert abs(float(loss) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach())) + 1e-9
        assert torch.equal(grad, ref_in.grad)
    # into caller-owned buffers
    lo, go = torch.zeros((), device=gpu_device), torch.zeros_like(img)
    l2, g2 = l1_loss_and_grad(img, gt, loss_out=lo, grad_out=go)
    assert l2.data_ptr() == lo.data_ptr() and g2.data_ptr() == go.data_ptr() and torch.equal(go, ref_in.grad)


@pytest.mark.parametrize("K,shape", [(1, (3, 64, 64)), (3, (3, 512, 512)), (4, (3, 37, 53))])
def test_l1_of_the_frames_of_a_batch_in_one_launch(gpu_device, K, shape):
    """fr_l1_loss_grad_batch == K calls of fr_l1_loss_grad: the same loss BITS (same partial sums, same order) and the same
    gradients, repeatedly (the workspaces come back zeroed), and distinct workspaces are enforced."""
    from fateavatar_amd.loss import l1_loss_and_grad, l1_loss_and_grad_batch, l1_workspace
    g = torch.Generator(device="cpu").manual_seed(K + sum(shape))
    imgs = [torch.rand(shape, generator=g).to(gpu_device) for _ in range(K)]
    gts = [torch.rand(shape, generator=g).to(gpu_device) for _ in range(K)]
    for a, b in zip(imgs, gts):
        b.view(-1)[::5] = a.view(-1)[::5]
    ref = [l1_loss_and_grad(a, b) for a, b in zip(imgs, gts)]
    losses = [torch.zeros((), device=gpu_device) for _ in range(K)]
    grads = [torch.full(shape, 7.0, device=gpu_device) for _ in range(K)]
    wss = [l1_workspace(gpu_device) for _ in range(K)]
    for _ in range(3):
        l1_loss_and_grad_batch(imgs, gts, losses, grads, wss)
        torch.cuda.synchronize()
        for k in range(K):
            assert torch.equal(losses[k], ref[k][0]) and torch.equal(grads[k], ref[k][1])
    if K > 1:
        with pytest.raises(RuntimeError, match="one workspace per image"):
            l1_loss_and_grad_batch(imgs, gts, losses, grads, [wss[0]] * K)


def test_l1_gradient_drives_the_rasterizer_backward(gpu_device):
    """render.backward(grad) with the fused gradient = l1_loss(render, gt).backward(): same parameter gradients."""
    from fateavatar_amd import scenes
    from fateavatar_amd.loss import l1_loss_and_grad
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render
    s = scenes.head_scene(P=5000, res=128, sh_degree=1, seed=2, opacity=0.5)
    cam = TorchCamera(s.camera, gpu_device)
    gt = torch.rand((3, 128, 128), device=gpu_device)
    bg = torch.ones(3, device=gpu_device)
    grads = []
    for fused in (False, True):
        pc = FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, s.sh_degree, gpu_device)
        pc.begin_step()
        out = render(cam, pc, bg)
        if fused:
            _, g = l1_loss_and_grad(out["render"], gt)
            out["render"].backward(g)
        else:
            torch.nn.functional.l1_loss(out["render"], gt).backward()
        grads.append(pc.collect_grads().clone())
    assert float(grads[0].abs().max()) > 0
    # (the blend backward sums with float atomics: two runs agree to rounding, not bit for bit)
    assert torch.allclose(grads[0], grads[1], rtol=1e-4, atol=1e-9)


def test_multi_copy(gpu_device):
    from fateavatar_amd.loss import multi_copy
    rng = np.random.default_rng(0)
    sizes = [35, 3 * 64 * 64, 5023 * 3, 1]
    src = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(gpu_device) for n in sizes]
    dst = [torch.zeros(n, device=gpu_device) for n in sizes]
    multi_copy(list(zip(dst, src)))
    for d, s in zip(dst, src):
        assert torch.equal(d, s)
    # unaligned views fall back to scalar copies inside the kernel
    big = torch.zeros(1000, device=gpu_device)
    multi_copy([(big[1:36], src[0])])
    assert torch.equal(big[1:36], src[0]) and float(big[0]) == 0 and float(big[36]) == 0
    with pytest.raises(RuntimeError):
        multi_copy([(dst[0], src[1])])


def test_scaled_sum(gpu_device):
    from fateavatar_amd.loss import scaled_sum
    g = torch.Generator().manual_seed(3)
    for n in (1 << 20, 1001):
        srcs = [torch.randn(n, generator=g).to(gpu_device) for _ in range(3)]
        dst = torch.empty(n, device=gpu_device)
        for k in (1, 2, 3):
            scaled_sum(dst, srcs[:k], 1.0 / k)
            want = srcs[0].clone()
            for t in srcs[1:k]:
                want = want + t
            assert torch.equal(dst, want * (1.0 / k))
        a = srcs[0].clone()
        scaled_sum(a, [a, srcs[1]], 0.5)            # in place
        assert torch.equal(a, (srcs[0] + srcs[1]) * 0.5)
    with pytest.raises(RuntimeError):
        scaled_sum(dst, [srcs[0][:10]], 1.0)


POISON = -12345.5


def _guarded(count, offset_words, dev):
    """A destination of `count` floats inside a larger poisoned buffer, `offset_words` floats past a 16-byte boundary."""
    front = 64 + offset_words
    whole = torch.full((front + count + 67,), POISON, device=dev)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[front:front + count]


def _source(count, offset_words, rng, dev):
    whole = torch.from_numpy(rng.standard_normal(64 + offset_words + count).astype(np.float32)).to(dev)
    return whole[64 + offset_words:]


COPY_COUNTS = [0, 1, 2, 3, 5, 4096, 0, 2048 * 256 * 4 + 4099, 4, 0, 1001, 600_001]


@pytest.mark.parametrize("misaligned", ["neither", "source", "destination", "both", "mixed"])
def test_multi_copy_twelve_segments_inside_guard_words(gpu_device, misaligned):
    """All 12 segments of one launch (through the C ABI, so that EMPTY segments between full ones reach the kernel): counts
    0, 1, 2, 3, 5, 4 096, one above what the launch's grid covers in one trip (2 048 x 256 float4) and one above it on
    the scalar path; source misaligned only, destination only, both, and a different misalignment per segment.  Every
    destination sits inside a larger poisoned buffer whose other words are untouched afterwards."""
    import ctypes as C
    from fateavatar_amd import _lib
    assert len(COPY_COUNTS) == 12 and max(COPY_COUNTS) > 2048 * 256 * 4
    rng = np.random.default_rng(len(misaligned))
    offs = {"neither": lambda i: (0, 0), "source": lambda i: (1 + i % 3, 0), "destination": lambda i: (0, 1 + i % 3),
            "both": lambda i: (1 + i % 3, 1 + (i + 1) % 3), "mixed": lambda i: (i % 4, (i // 4 + i) % 4)}[misaligned]
    srcs, wholes, dsts = [], [], []
    for i, n in enumerate(COPY_COUNTS):
        so, do = offs(i)
        srcs.append(_source(n, so, rng, gpu_device))
        w, d = _guarded(n, do, gpu_device)
        wholes.append(w), dsts.append(d)
        assert n == 0 or (srcs[-1].data_ptr() % 16 == 4 * so and d.data_ptr() % 16 == 4 * do)
    k = len(COPY_COUNTS)
    rc = _lib.lib().fr_multi_copy(k, (C.c_void_p * k)(*[d.data_ptr() for d in dsts]), (C.c_void_p * k)(*[s_.data_ptr() for s_ in srcs]),
                                  (C.c_uint64 * k)(*COPY_COUNTS), torch.cuda.current_stream(gpu_device).cuda_stream)
    assert rc == _lib.FR_OK, _lib.last_error()
    torch.cuda.synchronize()
    for i, (n, s_, w, d) in enumerate(zip(COPY_COUNTS, srcs, wholes, dsts)):
        assert torch.equal(d, s_), (i, n)
        front = w.numel() - n - 67
        assert bool((w[:front] == POISON).all()) and bool((w[front + n:] == POISON).all()), (i, n)
    # the same through multi_copy() (which drops the empty pairs itself), into fresh destinations
    again = [_guarded(n, offs(i)[1], gpu_device) for i, n in enumerate(COPY_COUNTS)]
    from fateavatar_amd.loss import multi_copy
    multi_copy([(d, s_) for (_, d), s_ in zip(again, srcs)])
    for i, (n, s_, (w, d)) in enumerate(zip(COPY_COUNTS, srcs, again)):
        assert torch.equal(d, s_), (i, n)
        front = w.numel() - n - 67
        assert bool((w[:front] == POISON).all()) and bool((w[front + n:] == POISON).all()), (i, n)


def test_multi_copy_refuses_thirteen_segments(gpu_device):
    import ctypes as C
    from fateavatar_amd import _lib
    from fateavatar_amd.loss import multi_copy
    src = [torch.ones(8, device=gpu_device) for _ in range(13)]
    dst = [torch.zeros(8, device=gpu_device) for _ in range(13)]
    with pytest.raises(RuntimeError, match="twelve"):
        multi_copy(list(zip(dst, src)))
    rc = _lib.lib().fr_multi_copy(13, (C.c_void_p * 13)(*[d.data_ptr() for d in dst]), (C.c_void_p * 13)(*[s_.data_ptr() for s_ in src]),
                                  (C.c_uint64 * 13)(*[8] * 13), torch.cuda.current_stream(gpu_device).cuda_stream)
    assert rc != _lib.FR_OK
    torch.cuda.synchronize()
    assert all(float(d.abs().max()) == 0.0 for d in dst)
    multi_copy(list(zip(dst[:12], src[:12])))
    assert all(torch.equal(d, s_) for d, s_ in zip(dst[:12], src[:12])) and float(dst[12].abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4096 * 256 * 4 + 4099])
def test_scaled_sum_small_counts_the_grid_stride_loop_and_in_place(gpu_device, n):
    """Counts 1, 2, 3, 5 (scalar tail only) and one above what the launch's grid covers in one trip (4 096 x 256 float4),
    K = 1 .. 4, and in place with dst being each of the sources in turn.  Expected: the float32 expression in the
    kernel's order, bit for bit; the words behind dst stay as they were."""
    from fateavatar_amd.loss import scaled_sum
    g = torch.Generator().manual_seed(n % 1000)
    srcs = [torch.randn(n, generator=g).to(gpu_device) * (10.0 ** (k - 1)) for k in range(4)]

    def expected(ts, scale):
        want = ts[0].clone()
        for t in ts[1:]:
            want = want + t
        return want * scale

    for K in (1, 2, 3, 4):
        scale = 1.0 / K
        whole = torch.full((n + 64,), POISON, device=gpu_device)
        scaled_sum(whole[:n], srcs[:K], scale)
        assert torch.equal(whole[:n], expected(srcs[:K], scale)) and bool((whole[n:] == POISON).all()), K
        for j in range(K):                              # dst is source j
            work = [t.clone() for t in srcs[:K]]
            want = expected(work, scale)
            scaled_sum(work[j], work, scale)
            assert torch.equal(work[j], want), (K, j)
            for i in range(K):
                assert i == j or torch.equal(work[i], srcs[i])


def test_concurrent_streams_overlap(gpu_device):
    """fateavatar_amd.streams: the runtime maps streams onto a few hardware queues; streams on one queue are serialised.
    concurrent_streams() returns streams that overlap pairwise and with the caller's stream."""
    from fateavatar_amd.streams import _overlap, concurrent_streams
    cur = torch.cuda.current_stream(gpu_device)
    ss = concurrent_streams(3, gpu_device, also_with=[cur])
    assert len(ss) == 3 and len({s.cuda_stream for s in ss}) == 3
    for i, a in enumerate(ss):
        assert _overlap(cur, a, gpu_device, 400_000)
        for b in ss[i + 1:]:
            assert _overlap(a, b, gpu_device, 400_000) and _overlap(b, a, gpu_device, 400_000)


@pytest.mark.gpu
def test_l1_losses_of_overlapping_launches_do_not_mix(gpu_device):
    """The loss kernel elects its last workgroup and sums per-workgroup partials through its workspace: launches that
    overlap (the lanes of AvatarBatchStep, one stream each) must each have their own (loss.py keeps one per stream)."""
    import torch
    from fateavatar_amd.loss import l1_loss_and_grad, l1_workspace
    torch.manual_seed(0)
    K, n_rep = 3, 40
    imgs = [torch.rand(3, 512, 512, device=gpu_device) for _ in range(K)]
    gts = [torch.rand(3, 512, 512, device=gpu_device) * (k + 1) for k in range(K)]
    want = [float((a - b).abs().mean()) for a, b in zip(imgs, gts)]
    streams = [torch.cuda.Stream(device=gpu_device) for _ in range(K)]
    losses = [[torch.zeros((), device=gpu_device) for _ in range(n_rep)] for _ in range(K)]
    explicit = [l1_workspace(gpu_device) for _ in range(K)]
    for mode in ("per-stream default", "explicit"):
        for s in streams:
            s.wait_stream(torch.cuda.current_stream(gpu_device))
        for r in range(n_rep):
            for k in range(K):
                with torch.cuda.stream(streams[k]):
                    l1_loss_and_grad(imgs[k], gts[k], loss_out=losses[k][r], workspace=explicit[k] if mode == "explicit" else None)
        torch.cuda.synchronize()
        for k in range(K):
            got = torch.stack(losses[k]).cpu().numpy()
            assert np.allclose(got, want[k], rtol=1e-5), (mode, k, got.min(), got.max(), want[k])
