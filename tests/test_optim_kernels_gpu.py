"""GPU: csrc/optim.hip (`opt_grad_norm`, `opt_step`) driven directly on flat buffers, against torch's own optimizers on the CPU.

Reference: the same numbers as three ``torch.nn.Parameter`` (one per group) in float64, stepped by
``GradScaler.unscale_`` -> ``torch.nn.utils.clip_grad_norm_`` -> ``torch.optim.{SGD(nesterov), AdamW, Adam}.step`` ->
``GradScaler.update`` -> EMA (ema = d * ema + (1 - d) * p, also for the float buffers), the order of the trainer's
optimizer_step.  The float32 run of the same program gives ``e_ref`` (tests/_kernel_ref.py).

Hyper-parameters reach the kernel as f32 fields of ``sy11_opt_desc``; the reference is given the same f32-rounded values
(0.999 as f32 is 0.99900001287..., and 1 - beta2 differs from 0.001 by 1.3e-5 relative: an input rounding, not a kernel error).

GradScaler: ``torch.amp.GradScaler("cpu")`` works with the installed torch (2.10) on float64 parameters, so it IS the reference
stepper of the AMP test, and `_scaler_update` below (a restatement of its documented update rule) is cross-checked against it
in the same test before the device values are compared.
"""
import numpy as np
import pytest
import torch

from tests._kernel_ref import DEV, Bars, lib, ops, rnd, same_bits

pytestmark = pytest.mark.gpu
F32 = torch.float32


def f32r(v):
    return float(np.float32(v))


LR = [f32r(v) for v in (0.01, 0.02, 0.005)]
MOM = [f32r(v) for v in (0.937, 0.9, 0.8)]
WD = [0.0, f32r(5e-4), f32r(1e-2)]
BETA2, EPS, DECAY = f32r(0.999), f32r(1e-8), f32r(0.9)

# (n, group ends): ends are multiples of 4.  1020: a boundary at float4 #100, inside the first workgroup's 256-float4 stride;
# 16388: an EMPTY middle group and a last group of one float4 past 4 full workgroup strides; 3000004: > 2048 workgroups' worth
LAYOUTS = {4: (4, 4, 4), 1020: (400, 1000, 1020), 4096 * 4 + 4: (4096 * 4, 4096 * 4, 4096 * 4 + 4), 3000004: (1000000, 2999996, 3000004)}


class CpuTrainer:
    """Three parameters (one per group), the torch optimizer of `kind`, optional GradScaler, EMA: one dtype."""

    def __init__(self, dt, p0, ends, kind, ema, buf, amp=None):
        b = [0, *ends]
        self.dt, self.b, self.ema_on = dt, b, ema
        self.params = [torch.nn.Parameter(p0[b[k]:b[k + 1]].to(dt).clone()) for k in range(3)]
        groups = []
        for k in range(3):
            g = {"params": [self.params[k]], "lr": LR[k], "weight_decay": WD[k]}
            g.update({"momentum": MOM[k], "nesterov": True} if kind == 0 else {"betas": (MOM[k], BETA2), "eps": EPS})
            groups.append(g)
        self.opt = (torch.optim.SGD(groups, lr=LR[0], momentum=MOM[0], nesterov=True) if kind == 0 else
                    (torch.optim.AdamW if kind == 1 else torch.optim.Adam)(groups, lr=LR[0]))
        self.ema = p0.to(dt).clone() if ema else None
        self.buf = buf.to(dt) if buf is not None else None
        self.ema_buf = torch.zeros_like(self.buf) if buf is not None else None
        self.scaler = None
        if amp:
            self.scaler = torch.amp.GradScaler("cpu", init_scale=amp["scale"], growth_factor=amp["growth"], backoff_factor=amp["backoff"],
                                               growth_interval=amp["interval"])
            self.scaler.scale(torch.tensor(1.0))                       # allocates the scale / tracker tensors
        self.steps_taken = 0

    def flat(self):
        return torch.cat([p.detach() for p in self.params])

    def state(self, name):
        """Flat optimizer state; zero where the optimizer has not created it (no step yet, or an empty parameter)."""
        out = []
        for p in self.params:
            st = self.opt.state.get(p, {})
            out.append(st[name].detach() if name in st and st[name] is not None else torch.zeros_like(p))
        return torch.cat(out)

    def step(self, grad_scaled, max_norm=10.0):
        """grad_scaled: flat f32 gradient as it sits in the device buffer (true gradient x loss scale).  -> (norm, skipped)."""
        for k, p in enumerate(self.params):
            p.grad = grad_scaled[self.b[k]:self.b[k + 1]].to(self.dt).clone()
        if self.scaler:
            self.scaler.unscale_(self.opt)
        norm = torch.nn.utils.clip_grad_norm_(self.params, max_norm=max_norm)
        skipped = False
        if self.scaler:
            skipped = sum(v.item() for v in self.scaler._per_optimizer_states[id(self.opt)]["found_inf_per_device"].values()) > 0
            self.scaler.step(self.opt)
            self.scaler.update()
        else:
            self.opt.step()
        self.steps_taken += 0 if skipped else 1
        self.opt.zero_grad()
        if self.ema_on:
            d = DECAY
            self.ema = d * self.ema + (1 - d) * self.flat()
            if self.buf is not None:
                self.ema_buf = d * self.ema_buf + (1 - d) * self.buf
        return norm.detach(), skipped


class GpuTrainer:
    def __init__(self, p0, ends, kind, ema, buf, amp=None):
        n = p0.numel()
        z = lambda: torch.zeros(n, dtype=F32, device=DEV)                      # noqa: E731
        self.n, self.ends, self.kind, self.amp = n, ends, kind, amp
        self.param, self.grad, self.mom, self.sq = p0.to(DEV).clone(), z(), z(), z()
        self.ema = p0.to(DEV).clone() if ema else None
        self.buf = buf.to(DEV) if (buf is not None and ema) else None
        self.ema_buf = torch.zeros_like(self.buf) if self.buf is not None else None
        self.ws = ops().opt_workspace(DEV)
        self.adam_step = torch.zeros(1, dtype=F32, device=DEV)
        self.norm_out = torch.full((2,), -1.0, dtype=F32, device=DEV)
        self.scale = torch.tensor([amp["scale"]], dtype=F32, device=DEV) if amp else None
        self.tracker = torch.zeros(1, dtype=torch.int32, device=DEV) if amp else None

    def step(self, grad_scaled, max_norm=10.0):
        self.grad.copy_(grad_scaled)
        a = self.amp or {"growth": 2.0, "backoff": 0.5, "interval": 2000}
        ops().opt_step(self.param, self.grad, self.mom, self.sq, self.ema, self.buf, self.ema_buf, self.ws, self.ends, LR, MOM, WD, self.kind, DECAY,
                       max_norm=max_norm, beta2=BETA2, eps=EPS, scale=self.scale, growth_tracker=self.tracker, adam_step=self.adam_step,
                       growth=a["growth"], backoff=a["backoff"], interval=a["interval"], norm_out=self.norm_out)
        torch.cuda.synchronize()
        return self.norm_out.cpu()


def _grads(n, steps, norm, seed):
    """`steps` flat gradients of Euclidean norm `norm` (f32)."""
    out = []
    for s in range(steps):
        g = rnd(n, seed=seed + s).double()
        out.append((g * (norm / g.norm())).float())
    return out


def _compare(b, tag, gpu, c64, c32, kind, ema, nbuf):
    b.add(f"{tag} param", gpu.param, c64.flat(), c32.flat())
    if kind == 0:
        b.add(f"{tag} mom", gpu.mom, c64.state("momentum_buffer"), c32.state("momentum_buffer"))
    else:
        b.add(f"{tag} mom", gpu.mom, c64.state("exp_avg"), c32.state("exp_avg"))
        b.add(f"{tag} sq", gpu.sq, c64.state("exp_avg_sq"), c32.state("exp_avg_sq"))
    if ema:
        b.add(f"{tag} ema", gpu.ema, c64.ema, c32.ema)
        if nbuf:
            b.add(f"{tag} ema_buf", gpu.ema_buf, c64.ema_buf, c32.ema_buf)


@pytest.mark.parametrize("ema,nbuf", [(False, 0), (True, 0), (True, 3), (True, 70001)], ids=["noema", "ema", "ema-buf3", "ema-buf70001"])
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["sgd", "adamw", "adam"])
@pytest.mark.parametrize("n", list(LAYOUTS))
def test_opt_step_matches_torch_optimizers(n, kind, clip, ema, nbuf):
    """4 consecutive steps; ||g|| = 50 against max_norm 10 (clip active: every gradient is scaled by one factor) or ||g|| = 3."""
    ends = LAYOUTS[n]
    p0 = rnd(n, seed=1)
    buf = rnd(nbuf, seed=2, scale=3.0) if nbuf else None
    gpu = GpuTrainer(p0, ends, kind, ema, buf)
    c64, c32 = CpuTrainer(torch.float64, p0, ends, kind, ema, buf), CpuTrainer(F32, p0, ends, kind, ema, buf)
    b = Bars(f"opt_step n{n} kind{kind} {'clip' if clip else 'noclip'} ema{int(ema)} nbuf{nbuf}")
    for s, g in enumerate(_grads(n, 4, 50.0 if clip else 3.0, seed=10)):
        no = gpu.step(g)
        n64, _ = c64.step(g)
        n32, _ = c32.step(g)
        assert float(gpu.grad.abs().max()) == 0.0, "the gradient buffer is not zero after the step"
        assert no[1].item() == 0.0
        b.add(f"step{s} norm", no[:1], n64.reshape(1), n32.reshape(1))
        assert gpu.adam_step.item() == s + 1                      # counts the steps taken, whatever the optimizer
        if s in (0, 3):
            _compare(b, f"step{s}", gpu, c64, c32, kind, ema, nbuf)
    b.check()


def _scaler_update(scale, tracker, found_inf, growth, backoff, interval):
    """torch.amp.GradScaler.update as documented: a skipped step multiplies the scale by `backoff` and clears the tracker;
    `interval` consecutive clean steps multiply it by `growth` (unless that leaves f32's range) and clear the tracker."""
    if found_inf:
        return f32r(scale * backoff), 0
    tracker += 1
    if tracker == interval:
        grown = np.float32(scale) * np.float32(growth)
        return (float(grown) if np.isfinite(grown) else scale), 0
    return scale, tracker


@pytest.mark.parametrize("kind", [0, 1], ids=["sgd", "adamw"])
@pytest.mark.parametrize("n", [1020, 4096 * 4 + 4])
def test_amp_state_machine(n, kind):
    """8 scripted steps at scale 65536, growth_interval 3: clean x3 (scale doubles on the 3rd), one inf element (skip), one NaN in
    the last float4 of the last group (skip), clean x3 (doubles again).  Scale, tracker, found_inf and the Adam step count are
    exact; a skipped step leaves param / mom / sq bit-identical, zeroes the gradient and still moves the EMA."""
    with np.errstate(over="ignore"):
        ends = LAYOUTS[n]
        amp = {"scale": 65536.0, "growth": 2.0, "backoff": 0.5, "interval": 3}
        p0, buf = rnd(n, seed=1), rnd(3, seed=2)
        gpu = GpuTrainer(p0, ends, kind, True, buf, amp)
        c64, c32 = (CpuTrainer(dt, p0, ends, kind, True, buf, amp) for dt in (torch.float64, F32))
        script = ["clean", "clean", "clean", "inf", "nan", "clean", "clean", "clean"]
        grads = _grads(n, len(script), 50.0, seed=30)
        scale, tracker, taken = amp["scale"], 0, 0
        b = Bars(f"amp n{n} kind{kind}")
        for s, what in enumerate(script):
            g = grads[s] * gpu.scale.item()                       # what backward leaves in the buffer: gradient x current scale
            if what == "inf":
                g[n // 3] = float("inf")
            elif what == "nan":
                g[n - 2] = float("nan")
            before = [t.clone() for t in (gpu.param, gpu.mom, gpu.sq, gpu.adam_step)]
            no = gpu.step(g)
            n64, skip64 = c64.step(g)
            n32, _ = c32.step(g)
            bad = what != "clean"
            scale, tracker = _scaler_update(scale, tracker, bad, amp["growth"], amp["backoff"], amp["interval"])
            taken += 0 if bad else 1
            # the restatement against torch's own scaler on the CPU, then the device against the restatement
            assert skip64 == bad and c64.scaler.get_scale() == scale and int(c64.scaler._growth_tracker.item()) == tracker and c64.steps_taken == taken
            assert gpu.scale.item() == scale, (s, what, gpu.scale.item(), scale)
            assert gpu.tracker.item() == tracker, (s, what, gpu.tracker.item(), tracker)
            assert no[1].item() == (1.0 if bad else 0.0), (s, what)
            assert gpu.adam_step.item() == taken, (s, what, gpu.adam_step.item())
            assert float(gpu.grad.abs().max()) == 0.0 and not bool(torch.isnan(gpu.grad).any()), f"step {s} ({what}): gradient not zeroed"
            if bad:
                for t0, t1, name in zip(before, (gpu.param, gpu.mom, gpu.sq, gpu.adam_step), ("param", "mom", "sq", "adam_step")):
                    assert same_bits(t0, t1), f"step {s} ({what}): {name} changed on a skipped step"
                b.add(f"step{s}({what}) ema", gpu.ema, c64.ema, c32.ema)
                b.add(f"step{s}({what}) ema_buf", gpu.ema_buf, c64.ema_buf, c32.ema_buf)
            else:
                b.add(f"step{s} norm", no[:1], n64.reshape(1), n32.reshape(1))
        assert scale == 65536.0 and tracker == 0 and taken == 6          # x2, /2, /2, x2
        _compare(b, "end", gpu, c64, c32, kind, True, 3)
        b.check()


def test_amp_growth_that_overflows_leaves_the_scale():
    """scale 2^127, growth 2 -> inf in f32: the scale stays, the tracker is cleared (optim.hip, GradScaler.update)."""
    n, ends = 1020, LAYOUTS[1020]
    amp = {"scale": 2.0 ** 127, "growth": 2.0, "backoff": 0.5, "interval": 1}
    gpu = GpuTrainer(rnd(n, seed=1), ends, 0, False, None, amp)
    no = gpu.step(torch.zeros(n))                                   # a clean (all-zero) gradient
    with np.errstate(over="ignore"):
        assert _scaler_update(amp["scale"], 0, False, 2.0, 0.5, 1) == (2.0 ** 127, 0)
    assert gpu.scale.item() == 2.0 ** 127 and gpu.tracker.item() == 0 and no[1].item() == 0.0
    amp["scale"] = 2.0 ** 126                                       # one below: the growth fits and is taken
    gpu = GpuTrainer(rnd(n, seed=1), ends, 0, False, None, amp)
    gpu.step(torch.zeros(n))
    assert gpu.scale.item() == 2.0 ** 127 and gpu.tracker.item() == 0


@pytest.mark.parametrize("n", [4, 1020, 4096 * 4 + 4, 3000004])
@pytest.mark.parametrize("scale", [None, 1024.0], ids=["noamp", "scale1024"])
def test_opt_grad_norm_partials(n, scale):
    """The per-workgroup partials, summed on the host in float64, are ||g / scale||^2; the header carries 1 / scale and the Adam
    step; two calls give bit-identical partials (fixed slots, fixed fold order, no atomics)."""
    o, nparts = ops(), ops().OPT_PARTS
    g = rnd(n, seed=3, scale=7.0)
    g_d = g.to(DEV)
    sc = torch.tensor([scale], dtype=F32, device=DEV) if scale else None
    st = torch.tensor([5.0], dtype=F32, device=DEV)
    runs = []
    for _ in range(2):
        ws = torch.full((4 + nparts,), -1.0, dtype=F32, device=DEV)
        lib().call("sy11_opt_grad_norm", n, o._p(g_d), o._p(sc), o._p(st), o._p(ws), nparts, o._stream())
        torch.cuda.synchronize()
        runs.append(ws.cpu())
    assert same_bits(runs[0], runs[1]), "opt_grad_norm is not reproducible"
    ws = runs[0]
    assert ws[0].item() == f32r(1.0 / (scale or 1.0)) and ws[1].item() == 5.0
    assert same_bits(g_d, g), "opt_grad_norm modified the gradient"
    inv = 1.0 / (scale or 1.0)
    b = Bars(f"opt_grad_norm n{n}")
    b.add("sum of partials", ws[4:].double().sum().reshape(1), ((g.double() * inv) ** 2).sum().reshape(1), ((g * inv) ** 2).sum().reshape(1))
    b.check()
