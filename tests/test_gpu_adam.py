"""k_adam (fr_optim.hip) against float64, one step at a time.

The measure is a ONE-STEP RESIDUAL: before a step the kernel's own param / exp_avg / exp_avg_sq and the gradient buffers are
cloned, the step is computed in float64 from the clones with the exact bias corrections 1 - beta^t, and what the kernel
wrote is compared with that.  The random walk a trajectory accumulates stays out of the comparison, so the bounds are
derived, not tuned (u = 2^-24, the float32 unit roundoff; g = grad_scale x the float64 sum of the buffers):

  exp_avg     |got - want| <= 4 u (|beta1 m| + |(1 - beta1) g|)
  exp_avg_sq  |got - want| <= 5 u want
  param       |got - want| <= ulp(param) / 2 + 16 u S,
              S = lr / (1 - beta1^t) (|beta1 m| + |(1 - beta1) g|) / (sqrt(v') / sqrt(1 - beta2^t) + eps)

16 counts the float32 roundings on the path from g to the update (scale; two products and a sum for m; three and a sum
for v; sqrt; 1 / sqrt(bc2) and its product; + eps; the divide; lr / bc1; the last product), rounded up; a numpy float32
emulation of correctly rounded arithmetic stays below 5.7.

A step on the sum of K buffers adds K - 1 float32 additions, each within u of the sum of the buffers' MAGNITUDES (the sum
itself may cancel): g is off by at most dg = (K - 1) u grad_scale sum |g_k| before anything else happens.  To first order
that moves exp_avg by (1 - beta1) dg, exp_avg_sq by (1 - beta2) (2 |g| dg + dg^2) and the update by dg |d update / d g|,
  |d update / d g| <= lr / bc1 ((1 - beta1) / denom + |m'| (1 - beta2) |g| / (sqrt(v') sqrt(bc2) denom^2)),
and these are added to the bounds above (they vanish for K = 1).

What the reference takes from the configuration, not from the kernel: the learning rates and grad_scale as the float32
values the C ABI carries, beta1 / beta2 / eps as its doubles; the per-element rate is rebuilt here from the segment list.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BETAS, EPS = (0.9, 0.999), 1e-8
LRS = dict(xyz=1.6e-4, feature_dc=2.5e-3, feature_rest=2.5e-3 / 20, opacity=0.05, scaling=5e-3, rotation=1e-3)
GRID_CAP = 2048 * 256 * 4          # elements one trip of k_adam's grid-stride loop covers at the launch's cap


def f32(x):
    return float(np.float32(x))


def element_lrs(segments, n, dev):
    """float64 [n]: element e of a (count, lr, period, split, lr2) run has lr if e % period < split else lr2."""
    lr = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    off = 0
    for seg in segments:
        cnt = int(seg[0])
        if len(seg) == 5 and seg[2]:
            e = torch.arange(cnt, device=dev)
            two = torch.tensor([f32(seg[1]), f32(seg[4])], dtype=torch.float64, device=dev)
            lr[off:off + cnt] = two[(e % int(seg[2]) >= int(seg[3])).long()]
        else:
            lr[off:off + cnt] = f32(seg[1])
        off += cnt
    assert off == n and not bool(torch.isnan(lr).any())
    return lr


def half_ulp(x64):
    """Half a float32 ulp at |x| (x in float64)."""
    _, e = torch.frexp(x64.abs().clamp(min=2.0 ** -126))        # |x| = f 2^e, f in [0.5, 1): ulp = 2^(e - 24)
    return torch.ldexp(torch.ones_like(x64), e - 25)


class Checked:
    """A FusedAdam whose every step is checked: residuals on EVERY element, the step count, the done-counters."""

    def __init__(self, n, segments, dev, grad_scale=1.0, seed=0, betas=BETAS, eps=EPS):
        from fateavatar_amd.optim import FusedAdam
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.n, self.dev, self.segments = n, dev, segments
        self.flat = torch.randn(n, device=dev, generator=self.gen)
        self.grad = torch.zeros(n, device=dev)
        self.opt = FusedAdam(self.flat, self.grad, segments, betas=betas, eps=eps, grad_scale=grad_scale)
        self.lr = element_lrs(segments, n, dev)
        self.b1, self.b2, self.eps, self.scale = float(betas[0]), float(betas[1]), float(eps), f32(grad_scale)
        self.t = 0
        # any done-counter word that was non-zero after ANY launch stays set here (no synchronisation per step)
        self.counters_seen = torch.zeros(self.opt.state.numel() - 32, dtype=torch.int32, device=dev)

    def blocks(self):
        return min(2048, ((self.n + 3) // 4 + 255) // 256)

    def random_grad(self, step, out=None):
        """As in test_fused_adam_matches_torch_adam: magnitudes from 1e-3 to 1e2, every seventh element zero."""
        g = torch.randn(self.n, device=self.dev, generator=self.gen) * (10.0 ** (step % 6 - 3))
        g[::7] = 0.0
        return g if out is None else out.copy_(g)

    def plain_step(self, grads=None):
        self.opt.step(grads)
        self.t += 1
        self.counters_seen |= self.opt.state[32:].view(torch.int32)

    def checked_step(self, grads=None, what="", check=True):
        """One step; returns {array: (worst residual in u, elements over the bound)}.  check=False only measures."""
        opt = self.opt
        bufs = [opt.grad] if grads is None else list(grads)
        p, m, v = (x.clone().double() for x in (opt.param, opt.exp_avg, opt.exp_avg_sq))
        g, gmag = torch.zeros_like(p), torch.zeros_like(p)
        for b in bufs:
            g += b.double()
            gmag += b.double().abs()
        self.plain_step(grads)
        t, b1, b2, K = self.t, self.b1, self.b2, len(bufs)
        g *= self.scale
        dg = (K - 1) * U * self.scale * gmag
        del gmag
        m_terms = (b1 * m).abs() + ((1 - b1) * g).abs()
        want_m = b1 * m + (1 - b1) * g
        want_v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        denom = want_v.sqrt() / np.sqrt(bc2) + self.eps
        want_p = p - self.lr / bc1 * want_m / denom
        S = self.lr / bc1 * m_terms / denom
        # what the K - 1 extra additions may cost (zero for K = 1), and the half ulp of the stored parameter
        slope = (1 - b1) / denom + want_m.abs() * (1 - b2) * g.abs() / (want_v.sqrt().clamp(min=1e-300) * np.sqrt(bc2) * denom * denom)
        free_m, free_v = (1 - b1) * dg, (1 - b2) * (2 * g.abs() * dg + dg * dg)
        free_p = half_ulp(torch.maximum(want_p.abs(), opt.param.double().abs())) + self.lr / bc1 * slope * dg
        fig = {}
        # the figure printed and kept: the error beyond that allowance in units of u x the magnitude the bound scales with,
        # to be held against the 4, 5 and 16 of the bounds
        for name, got, want, unit, free, factor in (("exp_avg", opt.exp_avg, want_m, m_terms, free_m, 4),
                                                    ("exp_avg_sq", opt.exp_avg_sq, want_v, want_v, free_v, 5),
                                                    ("param", opt.param, want_p, S, free_p, 16)):
            err = (got.double() - want).abs()
            ratio = torch.where(unit > 0, (err - free).clamp(min=0) / (U * unit).clamp(min=1e-300), torch.zeros_like(err))
            fig[name] = (float(ratio.max()), int((err > free + factor * U * unit).sum()))
        state = opt.state.cpu()
        print(f"adam residual [{what}] n={self.n} K={K} t={t}: " +
              ", ".join(f"{k} {a:.2f} u ({b} over the bound)" for k, (a, b) in fig.items()) +
              f"; state {state[:3].tolist()}")
        if not check:
            return fig
        assert float(state[0]) == t, (what, t, state[:3])
        assert not bool(state[32:].view(torch.int32).any()), (what, t, "a done-counter was left non-zero")
        assert not bool(self.counters_seen.any()), (what, t, "a done-counter was non-zero after an earlier launch")
        for name, (worst, n_over) in fig.items():
            assert n_over == 0, (what, name, f"t={t}", f"{n_over} of {self.n} elements over the bound, worst {worst:.2f} u")
        return fig


def production_segments(P, tail=0):
    """The five runs TrainStep builds for FlatGaussians at SH degree 3 (train.py, the FusedAdam(...) call); `tail` more
    elements go to the last run."""
    M = 16
    return [(P * 3, LRS["xyz"]), (P * M * 3, LRS["feature_dc"], M * 3, 3, LRS["feature_rest"]), (P, LRS["opacity"]),
            (P * 3, LRS["scaling"]), (P * 4 + tail, LRS["rotation"])]


@pytest.mark.parametrize("tail", [0, 1, 2, 3])
@pytest.mark.parametrize("P", [100_000, 500_000])
def test_adam_production_sizes(gpu_device, P, tail):
    """n = P x 59 (5.9 M and 29.5 M parameters: 3 and 15 trips of the grid-stride loop) and + 1, 2, 3 for the scalar
    tail, eight steps."""
    segs = production_segments(P, tail)
    n = P * 59 + tail
    assert sum(s[0] for s in segs) == n and n > GRID_CAP
    c = Checked(n, segs, gpu_device, seed=P + tail)
    assert c.blocks() == 2048
    for step in range(8):
        c.random_grad(step, out=c.grad)
        c.checked_step(what=f"production P={P} tail={tail}")
    assert c.opt.step_count == 8


SIXTEEN = [(1, 3e-2), (6, 1e-3, 3, 3, 5e-5), (13, 2e-3), (36, 2.5e-3, 12, 3, 1.25e-4), (2, 7e-3), (81, 1e-3, 27, 3, 5e-5),
           (3, 4e-4), (96, 2.5e-3, 48, 3, 1.25e-4), (5, 9e-3), (7 * 9 + 3, 6e-3, 7, 2, 3e-4), (1001, 1.6e-4),
           (48 * 41 + 5, 2.5e-3, 48, 3, 1.25e-4), (4, 5e-2), (27 * 30 + 1, 1e-2, 27, 3, 1e-4), (2, 8e-3), (1, 2e-2)]


def test_adam_all_sixteen_segments(gpu_device):
    """All 16 segments, boundaries on every residue mod 4, two-rate runs with the periods of SH degrees 0 .. 3 (3, 12, 27,
    48; split 3) and one that divides nothing (7, split 2; the run ends inside a period), first and last run one element."""
    from fateavatar_amd import _lib
    assert len(SIXTEEN) == _lib.FR_ADAM_MAX_SEGMENTS and SIXTEEN[0][0] == 1 and SIXTEEN[-1][0] == 1
    ends = np.cumsum([s[0] for s in SIXTEEN])
    assert {int(e) % 4 for e in ends} == {0, 1, 2, 3}
    assert {s[2] for s in SIXTEEN if len(s) == 5} == {3, 7, 12, 27, 48}
    n = int(ends[-1])
    c = Checked(n, SIXTEEN, gpu_device, grad_scale=0.5, seed=16)
    lr = c.lr.cpu().numpy()
    assert len(np.unique(lr)) >= 15 and np.count_nonzero(np.diff(lr)) > 150   # (the rates really change, run to run and inside)
    for step in range(8):
        c.random_grad(step, out=c.grad)
        c.checked_step(what="16 segments")
    # the same runs far apart, so that boundaries also fall into later trips of the grid-stride loop
    big = [(s[0] + (60_000 * (s[2] if len(s) == 5 else 1) if s[0] > 1 else 0),) + tuple(s[1:]) for s in SIXTEEN]
    n = sum(s[0] for s in big)
    assert n > 4 * GRID_CAP and big[0][0] == 1 and big[-1][0] == 1
    c = Checked(n, big, gpu_device, grad_scale=0.5, seed=17)
    for step in range(3):
        c.random_grad(step, out=c.grad)
        c.checked_step(what="16 long segments")


@pytest.mark.parametrize("n", [2 * GRID_CAP + 4096, 100_003, GRID_CAP + 1026])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_adam_on_the_sum_of_several_buffers(gpu_device, K, n):
    """step(grads=[...]) with 1 .. 4 buffers against the float64 sum: above the grid-stride threshold and with a tail."""
    segs = [(n // 3, 1e-3), (n - n // 3 - 5, 2.5e-3, 12, 3, 1.25e-4), (5, 5e-2)]
    c = Checked(n, segs, gpu_device, grad_scale=1.0 / K, seed=K * 7 + n % 11)
    bufs = [torch.zeros(n, device=gpu_device) for _ in range(K)]
    c.grad.fill_(float("nan"))                            # the optimizer's own buffer is not read when grads are given
    for step in range(4):
        for k, b in enumerate(bufs):
            c.random_grad(step + k, out=b)                # (different magnitudes per buffer: the sum is not K x one)
        c.checked_step(grads=bufs, what=f"K={K}")


def test_adam_unused_gradient_slots_do_not_matter(gpu_device):
    """Two buffers, with two further allocations full of poison (NaN, 1e30) next to them: the result is what two buffers
    give, to the bit, whatever lies in memory where a third and a fourth would be."""
    n = GRID_CAP + 7
    runs = []
    for poison in (None, float("nan"), 1e30):
        c = Checked(n, [(n, 1e-3)], gpu_device, grad_scale=0.5, seed=5)
        bufs = [torch.zeros(n, device=gpu_device) for _ in range(2)]
        junk = None if poison is None else [torch.full((n,), poison, device=gpu_device) for _ in range(2)]
        for step in range(3):
            for k, b in enumerate(bufs):
                c.random_grad(step + k, out=b)
            c.checked_step(grads=bufs, what=f"K=2 poison={poison}")
        runs.append((c.flat.clone(), c.opt.exp_avg.clone(), c.opt.exp_avg_sq.clone()))
        del junk
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


CHECKPOINTS = (1, 2, 10, 100, 300, 1000, 3000, 10_000, 20_000)


def test_adam_long_run_keeps_the_bias_corrections_exact(gpu_device):
    """20 000 steps on 4 099 parameters, residuals at t = 1, 2, 10, 100, 300, 1 000, 3 000, 10 000, 20 000 and the step
    count at each.  The bias corrections 1 - beta^t come from a recurrence on the device; carried in float32 it drifts and,
    with beta2 = 0.999f, stops at 0.99997020 instead of reaching 1.

    Worst param residual beyond the half ulp of the stored value, in units of u x S (the bound is 16), and the number of
    the 4 099 elements over the bound, measured on an MI355X with this test's inputs:

        t                      1     2     10    100   300     1 000   3 000   10 000   20 000
        float32 recurrence     2.69  3.65  2.34  5.48  21.87   34.81   5.66    18.37    246.17
          elements over        0     0     0     0     22      32      0       1        207
        double recurrence      2.69  3.65  1.49  0.72  3.78    2.34    1.61    1.84     1.57
          elements over        0     0     0     0     0       0       0       0        0

    (float32: state[1..2] end at 0.99999976 and 0.99997020 instead of 1 and 1.  The error of the float32 sequence is not
    monotone in t, it is the sum of the roundings still alive, hence the dip at 3 000.)

    exp_avg and exp_avg_sq do not depend on the corrections and stay within their bounds in both."""
    n = 4099
    c = Checked(n, [(1000, 1.6e-4), (3000, 2.5e-3, 12, 3, 1.25e-4), (99, 5e-2)], gpu_device, seed=3)
    figs = {}
    for t in range(1, CHECKPOINTS[-1] + 1):
        c.random_grad(t, out=c.grad)
        if t in CHECKPOINTS:
            figs[t] = c.checked_step(what="long run")   # (synchronises; the steps between do not)
        else:
            c.plain_step()
    assert c.opt.step_count == CHECKPOINTS[-1]
    # the corrections a reader of the state sees are the float32 roundings of the exact ones
    s = c.opt.state[:3].cpu().double()
    for k, b in ((1, BETAS[0]), (2, BETAS[1])):
        assert abs(float(s[k]) - (1 - b ** CHECKPOINTS[-1])) <= U, (k, float(s[k]))
    print("long run, worst param residual in u x S:", {t: round(f["param"][0], 2) for t, f in figs.items()})


def test_adam_corrections_stay_exact_for_a_hundred_thousand_steps(gpu_device):
    """The state's corrections at t = 10^5 and at every power of ten before: within one float32 rounding of 1 - beta^t,
    and the doubles behind them (state words 4..7) within 1e-12."""
    c = Checked(8, [(8, 1e-3)], gpu_device, seed=1)
    c.grad.fill_(0.25)
    for t in range(1, 100_001):
        c.plain_step()
        if t in (1, 10, 100, 1000, 10_000, 100_000):
            head = c.opt.state[:3].cpu().double()
            carried = c.opt.state[4:8].cpu().view(torch.float64)
            assert float(head[0]) == t
            for k, b in enumerate(BETAS):
                exact = 1.0 - b ** t
                print(f"adam corrections t={t} beta={b}: float {float(head[1 + k])!r} double {float(carried[k])!r} exact {exact!r}")
                assert abs(float(head[1 + k]) - exact) <= U * exact
                assert abs(float(carried[k]) - exact) <= 1e-12
    assert not bool(c.counters_seen.any())


@pytest.mark.parametrize("n_words", [0, 1, 2, 3, 4])
def test_adam_skip_words(gpu_device, n_words):
    """0 .. 4 skip words, each position non-zero in turn: parameters, both moments and all state words unchanged to the
    bit, done-counters zero; with the word cleared the next step is step t + 1, not t + 2."""
    n = 70_001
    c = Checked(n, [(n - 3, 1e-3), (3, 5e-2)], gpu_device, seed=n_words)
    words = [torch.zeros(1, device=gpu_device) for _ in range(n_words)]
    c.opt.set_skip_words(words)
    for step in range(3):
        c.random_grad(step, out=c.grad)
        c.checked_step(what=f"{n_words} skip words, none set")
    for pos in range(n_words):
        for value in (1.0, float("nan")):
            before = [x.clone() for x in (c.flat, c.opt.exp_avg, c.opt.exp_avg_sq, c.opt.state)]
            words[pos].fill_(value)
            c.random_grad(pos, out=c.grad)
            c.opt.step()
            torch.cuda.synchronize()
            for a, b in zip(before, (c.flat, c.opt.exp_avg, c.opt.exp_avg_sq, c.opt.state)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (pos, value)
            assert c.opt.step_count == c.t and not bool(c.opt.state[32:].view(torch.int32).any())
            words[pos].zero_()
            c.checked_step(what=f"after a skipped step (word {pos} = {value})")   # asserts state[0] == t: t + 1, not t + 2


@pytest.mark.parametrize("blocks", [1, 15, 16, 17, 2048])
def test_adam_done_counters_return_to_zero(gpu_device, blocks):
    """The election of the last workgroup (16 group counters and a final one) leaves every counter at zero after every
    launch, at grid sizes on both sides of the group count and at the cap: a counter left behind corrupts the NEXT step's
    state hand-over, which a single launch never shows."""
    n = {1: 1000, 15: 15 * 1024 - 5, 16: 16 * 1024, 17: 16 * 1024 + 1, 2048: GRID_CAP + 4099}[blocks]
    c = Checked(n, [(n, 1e-3)], gpu_device, seed=blocks)
    assert c.blocks() == blocks
    for step in range(40):
        c.random_grad(step, out=c.grad)
        if step < 4 or step % 13 == 0:
            c.checked_step(what=f"{blocks} workgroups")
        else:
            c.plain_step()
    torch.cuda.synchronize()
    assert c.opt.step_count == 40 and not bool(c.counters_seen.any())
    c.checked_step(what=f"{blocks} workgroups, step 41")


def test_adam_graph_replay_equals_eager(gpu_device):
    """One captured step replayed 300 times == 300 eager launches, bit for bit, all 576 state words included."""
    n = 300_007
    segs = [(n - 7, 2.5e-3, 48, 3, 1.25e-4), (7, 5e-2)]
    eager, graphed = (Checked(n, segs, gpu_device, grad_scale=0.5, seed=9) for _ in range(2))
    assert torch.equal(eager.flat, graphed.flat)
    g = eager.random_grad(2)
    eager.grad.copy_(g)
    graphed.grad.copy_(g)
    for _ in range(300):
        eager.opt.step()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        graphed.opt.step()
    torch.cuda.synchronize()
    assert graphed.opt.step_count == 0                   # (capturing runs nothing)
    for _ in range(300):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in ((eager.flat, graphed.flat), (eager.opt.exp_avg, graphed.opt.exp_avg),
                 (eager.opt.exp_avg_sq, graphed.opt.exp_avg_sq), (eager.opt.state, graphed.opt.state)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert graphed.opt.step_count == 300 and not bool(graphed.opt.state[32:].view(torch.int32).any())
    eager.t = graphed.t = 300
    eager.checked_step(what="eager, step 301")
    graphed.checked_step(what="after 300 replays, step 301")


def test_adam_state_survives_a_checkpoint(gpu_device):
    """state_words() / load_state_words(): a restored optimizer continues bit for bit, and a four-word state (written
    before the corrections were carried as doubles) is completed from its step count."""
    n = 5003
    segs = [(n, 1e-3)]
    a = Checked(n, segs, gpu_device, seed=4)
    for step in range(1500):
        a.random_grad(step, out=a.grad)
        a.plain_step()
    words = a.opt.state_words()
    assert words.numel() == 8
    restored = []
    for keep in (8, 4):
        b = Checked(n, segs, gpu_device, seed=4)
        for dst, src in ((b.flat, a.flat), (b.opt.exp_avg, a.opt.exp_avg), (b.opt.exp_avg_sq, a.opt.exp_avg_sq), (b.grad, a.grad)):
            dst.copy_(src)
        b.opt.load_state_words(words[:keep])
        b.t = a.t
        assert b.opt.step_count == 1500 and torch.equal(b.opt.state[:4].view(torch.int32), a.opt.state[:4].view(torch.int32))
        d = (b.opt.state[4:8].cpu().view(torch.float64) - a.opt.state[4:8].cpu().view(torch.float64)).abs().max()
        assert float(d) == 0.0 if keep == 8 else float(d) < 1e-12
        restored.append(b)
    a.checked_step(what="uninterrupted, step 1501")
    for b, keep in zip(restored, (8, 4)):
        b.checked_step(what=f"restored from {keep} words, step 1501")
    # (bits, not values: half a double read as a float may be a NaN)
    assert torch.equal(a.flat, restored[0].flat) and torch.equal(a.opt.state.view(torch.int32), restored[0].opt.state.view(torch.int32))
