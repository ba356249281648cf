"""csrc/adam.hip pinned bit for bit, through the C ABI, in the regime the workload trains in.

Every output of the three entry points (anr_adam_step, anr_adam_step_multi,
anr_adam_step_multi_dev) -- the f32 parameters, both moments, the f16 shadow and the zeroed
gradient -- is compared with tests/adam_ref.py's scalar-order f32 emulation by bit pattern
(any NaN equal to any NaN). adam.hip is built without contraction and with f32 denormals
on, and its division and square root are the IEEE expansions, so nothing less than equality
is expected. The inputs are where eps = 1e-15 matters: tables in +-1e-4, sparse gradients
from 1e-24 up, g*g denormal or underflowing, overflow, inf / NaN, signed zeros
(adam_ref.edge_values, adam_ref.workload_grads; test_adam_ref_cpu.py shows that dropping
eps, moving it inside the square root or using 1e-8 changes over 1 % of these elements).

Every array lives inside a larger buffer of sentinels (at least 64 elements on each side)
and starts one element past a 16-byte boundary, as FusedAdam's shadows (views into a flat
f16 buffer at any element offset) and a flat gradient bucket's views do; after every call
the sentinels of p, g, m, v and the shadow must be unchanged.

What the device-step form's tick kernel computes with the device's double pow is compared
with the host's std::pow at steps 1, 2, 7, 100, 1000, 50000 (1 f32 ulp: a double result
under 1 ulp off, rounded once), and the update is held bit for bit to the emulation fed
the scalars the device produced.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import adam_ref as ar

pytestmark = pytest.mark.gpu

f32 = np.float32
B1, B2, EPS, LR = ar.HYPER["b1"], ar.HYPER["b2"], ar.HYPER["eps"], ar.HYPER["lr"]
MODE_IDS = [m[0] for m in ar.MODES]
STEPS6 = [1, 2, 7, 100, 1000, 50000]
SENTINEL = {4: 0xDEADBEEF, 2: 0xBEEF}
SIZES = [1, 255, 256, 1023, 1024, 1025, 4097]


class Guarded:
    """An array inside a sentinel-filled device buffer, one element past a 16-byte boundary."""

    def __init__(self, values, dev):
        values = np.ascontiguousarray(values)
        self.dtype, self.n, size = values.dtype, len(values), values.dtype.itemsize
        self.utype, self.itype = {4: (np.uint32, np.int32), 2: (np.uint16, np.int16)}[size]
        self.t = torch.empty(self.n + 64 + 8 + 64, dtype={4: torch.int32, 2: torch.int16}[size],
                             device=dev)
        base = self.t.data_ptr()
        self.lo = next(k for k in range(64, 72) if (base + k * size) % 16 == size)
        host = np.full(self.t.numel(), SENTINEL[size], self.utype)
        host[self.lo:self.lo + self.n] = values.view(self.utype)
        self.host = host
        self.t.copy_(torch.from_numpy(host.view(self.itype)))
        self.ptr = base + self.lo * size

    def set(self, values):
        v = np.ascontiguousarray(values, self.dtype).view(self.itype)
        assert len(v) == self.n
        self.t[self.lo:self.lo + self.n].copy_(torch.from_numpy(v))

    def read(self, what=""):
        """The array as the device holds it; the sentinels around it must be untouched."""
        now = self.t.cpu().numpy().view(self.utype)
        lo, hi = self.lo, self.lo + self.n
        assert (now[:lo] == self.host[:lo]).all(), f"{what}: written before the array"
        assert (now[hi:] == self.host[hi:]).all(), f"{what}: written past the array"
        return now[lo:hi].view(self.dtype).copy()


class Tensor:
    """One optimizer tensor on the device (p, g, m, v and optionally the shadow), guarded."""

    def __init__(self, dev, p, g, m, v, shadow=True):
        self.init = tuple(np.array(x, f32) for x in (p, g, m, v))
        self.p, self.g, self.m, self.v = (Guarded(x, dev) for x in self.init)
        # the shadow starts as garbage that the update must overwrite
        self.p16 = Guarded(np.full(len(p), 7.0, np.float16), dev) if shadow else None
        self.n = len(p)

    def desc(self, lr=LR, wd=0.0, step=1, gq=0.0):
        from atmonr_amd import _lib

        return _lib.AdamTensor(self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr,
                               self.p16.ptr if self.p16 else None, self.n, lr, wd, step, gq)

    def read(self, what=""):
        out = {k: getattr(self, k).read(f"{what} {k}") for k in ("p", "g", "m", "v")}
        out["p16"] = self.p16.read(f"{what} p16") if self.p16 else None
        return out

    def check(self, ref, zero_grad, what, g_before=None):
        """Against (p, m, v, p16) of the emulation, bit for bit; g zeroed or untouched."""
        got = self.read(what)
        for k, want in zip(("m", "v", "p"), (ref[1], ref[2], ref[0])):
            ar.assert_bits_equal(got[k], want, f"{what} {k}")
        if self.p16:
            ar.assert_bits_equal(got["p16"], ref[3], f"{what} shadow")
        if zero_grad:
            assert not got["g"].view(np.uint32).any(), f"{what}: g not all +0.0"
        else:
            ar.assert_bits_equal(got["g"].view(np.uint32),
                                 (self.init[1] if g_before is None else g_before).view(np.uint32),
                                 f"{what} g")
        return got

    def check_untouched(self, what):
        got = self.read(what)
        for k, x in zip(("p", "g", "m", "v"), self.init):
            assert (got[k].view(np.uint32) == x.view(np.uint32)).all(), f"{what} {k} written"
        if self.p16:
            assert (got["p16"] == np.float16(7.0)).all(), f"{what} shadow written"


def _array(ts):
    from atmonr_amd import _lib

    return (_lib.AdamTensor * len(ts))(*ts)


def _multi(descs, decoupled, zero_grad, dev):
    from atmonr_amd import _lib

    arr = _array(descs)
    _lib.call("anr_adam_step_multi", ctypes.addressof(arr), len(descs), B1, B2, EPS,
              int(decoupled), int(zero_grad), _lib.stream(dev))
    torch.cuda.synchronize()


def _single(t, lr, wd, decoupled, step, zero_grad, dev):
    from atmonr_amd import _lib

    _lib.call("anr_adam_step", t.p.ptr, t.g.ptr, t.m.ptr, t.v.ptr, t.p16.ptr if t.p16 else None,
              t.n, lr, B1, B2, EPS, wd, int(decoupled), step, int(zero_grad), _lib.stream(dev))
    torch.cuda.synchronize()


def _emulate(x, *, lr=LR, wd, decoupled, step, gq=0.0, scalars=None):
    p, g, m, v = x
    return ar.adam_step_f32(p, g, m, v, lr=lr, b1=B1, b2=B2, eps=EPS, wd=wd, decoupled=decoupled,
                            step=step, grad_quant=gq, scalars=scalars)


# ------------------------------------------------------------------ a. per-tensor form
@functools.lru_cache(maxsize=None)
def _edge_reference(mode, step):
    _, decoupled, wd = ar.MODES[mode]
    x = ar.edge_values(4099)
    return x, _emulate(x, wd=wd, decoupled=decoupled, step=step)


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("mode", range(3), ids=MODE_IDS)
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "noshadow"])
def test_per_tensor_step_on_edge_values(dev, shadow, zero_grad, mode, step):
    _, decoupled, wd = ar.MODES[mode]
    x, ref = _edge_reference(mode, step)
    t = Tensor(dev, *x, shadow=shadow)
    _single(t, LR, wd, decoupled, step, zero_grad, dev)
    t.check(ref, zero_grad, "anr_adam_step")


# ------------------------------------------------------------------ b. grid stride
def test_per_tensor_grid_stride(dev):
    """n = 8192*256 + 257: the grid is capped at 8192 blocks of 256 threads, so the last 257
    elements are the second trip of 257 threads. One AdamW step from the state two emulated
    steps leave, shadow written, gradient zeroed."""
    n = 8192 * 256 + 257
    rng = np.random.default_rng(5)
    p, grads = ar.workload_params(rng, n), ar.workload_grads(rng, n, 3)
    m, v = np.zeros(n, f32), np.zeros(n, f32)
    for k in (0, 1):
        p, m, v, _ = _emulate((p, grads[k], m, v), wd=1e-2, decoupled=True, step=k + 1)
    x = (p, grads[2], m, v)
    ref = _emulate(x, wd=1e-2, decoupled=True, step=3)
    t = Tensor(dev, *x)
    _single(t, LR, 1e-2, True, 3, 1, dev)
    got = t.check(ref, 1, "anr_adam_step grid stride")
    assert ar.bits_differ(got["p"][-257:], p[-257:]).mean() > 0.9  # the second trip ran


# ------------------------------------------------------------------ c. multi form
# the issue's placement (the launch of 16 non-empty tensors ends after descriptor 19), and
# one where the second launch begins on an empty descriptor (16 non-empty end at 17)
EMPTIES = {"empty_0_5_16_17_34": (0, 5, 16, 17, 34), "empty_0_5_18_19_34": (0, 5, 18, 19, 34)}
GQS = [0.0, 128.0, 1000.0, 0.5]


def _multi_case(dev, mode, empties, count=35, shadows=lambda t: t % 2 == 0):
    """descriptors' settings and guarded tensors: sizes cycle through SIZES, own lr / wd /
    step / grad_quant each, edge values (or workload values for the smallest)."""
    _, decoupled, wd0 = ar.MODES[mode]
    tensors, settings = [], []
    k = 0
    for t in range(count):
        n = 0 if t in empties else SIZES[k % len(SIZES)]
        k += n > 0
        x = ar.edge_values(n, seed=t)
        if 0 < n < 64:
            rng = np.random.default_rng(t)
            x = (x[0], ar.workload_grads(rng, n, 1)[0] + f32(1e-9), x[2], x[3])
        tensors.append(Tensor(dev, *x, shadow=shadows(t)))
        settings.append(dict(lr=float(f32(LR * (1.0 + 0.37 * t))),
                             wd=float(f32(wd0 * (1.0 + 0.1 * t))), step=STEPS6[t % 6],
                             gq=GQS[t % 4]))
    return decoupled, tensors, settings


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("empties", list(EMPTIES))
@pytest.mark.parametrize("mode", range(3), ids=MODE_IDS)
def test_multi_form_per_tensor_settings(dev, mode, empties, zero_grad):
    from atmonr_amd import _lib

    decoupled, tensors, settings = _multi_case(dev, mode, EMPTIES[empties])
    _multi([t.desc(**s) for t, s in zip(tensors, settings)], decoupled, zero_grad, dev)
    outs = []
    for i, (t, s) in enumerate(zip(tensors, settings)):
        ref = _emulate(t.init, decoupled=decoupled, **s)
        outs.append(t.check(ref, zero_grad, f"multi tensor {i} (n {t.n}, {s})"))
    # grad_quant in the update == anr_grad_quantize_f16, then the update without it
    _, again, _ = _multi_case(dev, mode, EMPTIES[empties])
    for i, (t, s) in enumerate(zip(again, settings)):
        if s["gq"] and t.n:
            _lib.call("anr_grad_quantize_f16", t.g.ptr, t.n, s["gq"], _lib.stream(dev))
    torch.cuda.synchronize()
    quantised = [t.g.read(f"quantize {i}") for i, t in enumerate(again)]
    for i, (t, s) in enumerate(zip(again, settings)):
        if s["gq"]:
            ar.assert_bits_equal(quantised[i], ar.quant_f16(t.init[1], s["gq"]), f"quantize {i}")
    _multi([t.desc(**{**s, "gq": 0.0}) for t, s in zip(again, settings)], decoupled, zero_grad, dev)
    for i, (t, s, first) in enumerate(zip(again, settings, outs)):
        second = t.read(f"quantize + multi {i}")
        for k in ("p", "m", "v", "p16"):
            if first[k] is not None:
                ar.assert_bits_equal(second[k], first[k], f"tensor {i} {k}: fused quantisation "
                                                          "against the separate pass")


@pytest.mark.parametrize("bad", [65504.0, -1.0])
def test_multi_form_refuses_bad_grad_quant(dev, bad):
    from atmonr_amd import _lib

    decoupled, tensors, settings = _multi_case(dev, 1, EMPTIES["empty_0_5_16_17_34"])
    settings[33]["gq"] = bad  # in the third launch's batch
    with pytest.raises(_lib.ANRError, match="tensor 33: bad grad_quant"):
        _multi([t.desc(**s) for t, s in zip(tensors, settings)], decoupled, 1, dev)
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        t.check_untouched(f"refused call, tensor {i}")


# ------------------------------------------------------------------ d. device-step form
DEV_EMPTIES = (0, 15, 16, 31, 63)


def _dev_call(descs, decoupled, zero_grad, d_step, d_lr, d_scratch, dev):
    from atmonr_amd import _lib

    arr = _array(descs)
    _lib.call("anr_adam_step_multi_dev", ctypes.addressof(arr), len(descs), B1, B2, EPS,
              int(decoupled), int(zero_grad), d_step, d_lr, d_scratch, _lib.stream(dev))
    torch.cuda.synchronize()


def _dev_state(dev, settings, step):
    d_step = torch.tensor([step - 1], dtype=torch.int64, device=dev)
    d_lr = Guarded(np.array([s["lr"] for s in settings], f32), dev)
    d_scratch = Guarded(np.full(3 * 64, -7.0, f32), dev)
    return d_step, d_lr, d_scratch


@pytest.mark.parametrize("step", STEPS6)
@pytest.mark.parametrize("mode", range(3), ids=MODE_IDS)
def test_device_step_form_64_tensors(dev, mode, step):
    """64 descriptors (four launches), empty ones shifting the launch slot against the
    caller's index; distinct d_lr[t] and wd, so a tensor reading another's scalars shows."""
    decoupled, tensors, settings = _multi_case(dev, mode, DEV_EMPTIES, count=64)
    d_step, d_lr, d_scratch = _dev_state(dev, settings, step)
    # the descriptors' own lr / step are not what this form reads
    descs = [t.desc(lr=123.0, wd=s["wd"], step=0, gq=s["gq"]) for t, s in zip(tensors, settings)]
    _dev_call(descs, decoupled, 1, d_step.data_ptr(), d_lr.ptr, d_scratch.ptr, dev)
    assert int(d_step.item()) == step
    ar.assert_bits_equal(d_lr.read("d_lr"), np.array([s["lr"] for s in settings], f32), "d_lr")
    scal = d_scratch.read("d_scratch").reshape(64, 3)
    host = np.array([ar.adam_scalars(s["lr"], B1, B2, s["wd"], step) for s in settings], f32)
    off = ar.ulp_distance(scal, host)
    differ = ar.bits_differ(scal, host)
    print(f"device scalars at step {step} ({MODE_IDS[mode]}): step_size differs from the host's in "
          f"{int(differ[:, 0].sum())} of 64, bc2_sqrt in {int(differ[:, 1].sum())}, decay in "
          f"{int(differ[:, 2].sum())}; largest {off.max():.2f} ulp")
    assert off.max() <= 1.0
    ar.assert_bits_equal(scal[:, 2], host[:, 2], "decay (no pow in it)")
    if step == 50000:  # both corrections are exactly 1 in double, whatever pow's last bit
        ar.assert_bits_equal(scal, host, "device scalars at step 50000")
    for i, (t, s) in enumerate(zip(tensors, settings)):
        ref = _emulate(t.init, decoupled=decoupled, wd=s["wd"], gq=s["gq"], step=step,
                       scalars=tuple(scal[i]))
        t.check(ref, 1, f"dev tensor {i} (n {t.n}, {s})")


def test_device_step_form_refusals(dev):
    from atmonr_amd import _lib

    decoupled, tensors, settings = _multi_case(dev, 1, DEV_EMPTIES, count=64)
    extra = Tensor(dev, *ar.edge_values(256, seed=99))
    d_step, d_lr, d_scratch = _dev_state(dev, settings + [settings[1]], 7)
    descs = [t.desc(lr=s["lr"], wd=s["wd"], step=0, gq=s["gq"]) for t, s in zip(tensors, settings)]
    args = dict(d_step=d_step.data_ptr(), d_lr=d_lr.ptr, d_scratch=d_scratch.ptr)
    cases = [(descs + [extra.desc()], args, "0..64 tensors")]
    cases += [(descs, {**args, k: None}, "null device state") for k in args]
    for ds, a, msg in cases:
        with pytest.raises(_lib.ANRError, match=msg):
            _dev_call(ds, decoupled, 1, a["d_step"], a["d_lr"], a["d_scratch"], dev)
    torch.cuda.synchronize()
    assert int(d_step.item()) == 6
    assert (d_scratch.read("d_scratch") == f32(-7.0)).all()
    for i, t in enumerate(tensors + [extra]):
        t.check_untouched(f"refused call, tensor {i}")


# ------------------------------------------------------------------ e. 20-step trajectory
@pytest.mark.parametrize("mode", range(3), ids=MODE_IDS)
def test_trajectory_multi_per_tensor_emulation_and_torch(dev, mode):
    """20 steps from zero state on workload gradients: the multi form, the per-tensor form
    and the chained emulation end in the same bits (p, m, v, shadow), and that state is
    within 4x torch-f32's own error of torch-f64 (the criterion of test_adam_ref_cpu.py)."""
    name, decoupled, wd = ar.MODES[mode]
    n, steps = 20011, 20
    rng = np.random.default_rng(11)
    p0, grads = ar.workload_params(rng, n), ar.workload_grads(rng, n, steps)
    zeros = np.zeros(n, f32)
    a, b = Tensor(dev, p0, grads[0], zeros, zeros), Tensor(dev, p0, grads[0], zeros, zeros)
    p, m, v = p0, zeros, zeros
    for k in range(steps):
        a.g.set(grads[k])
        b.g.set(grads[k])
        _multi([a.desc(wd=wd, step=k + 1)], decoupled, 0, dev)
        _single(b, LR, wd, decoupled, k + 1, 0, dev)
        p, m, v, p16 = _emulate((p, grads[k], m, v), wd=wd, decoupled=decoupled, step=k + 1)
    ga = a.check((p, m, v, p16), 0, "multi form after 20 steps", g_before=grads[-1])
    gb = b.check((p, m, v, p16), 0, "per-tensor form after 20 steps", g_before=grads[-1])
    for k in ("p", "m", "v", "p16"):
        ar.assert_bits_equal(ga[k], gb[k], f"multi against per-tensor, {k}")
    ref64 = ar.torch_trajectory(p0, grads, decoupled=decoupled, wd=wd, dtype=torch.float64)
    t32 = ar.torch_trajectory(p0, grads, decoupled=decoupled, wd=wd, dtype=torch.float32)
    gmax = ar.moment_gradient_max(p0, grads, decoupled=decoupled, wd=wd)
    kern = ar.trajectory_errors((ga["p"], ga["m"], ga["v"]), ref64, gmax, lr=LR, steps=steps)
    tor = ar.trajectory_errors(t32, ref64, gmax, lr=LR, steps=steps)
    print(f"{name}: kernel {kern}, torch f32 {tor}")
    for k in kern:
        assert kern[k] <= 4.0 * tor[k], (name, k, kern[k], tor[k])


# ------------------------------------------------------------------ f. FusedAdam
def test_fused_adam_shadow_zero_grad_and_moments_across_forms(dev):
    """FusedAdam(zero_grad_in_step=True) with _anr_shadow views into one flat f16 buffer at
    odd element offsets, in its three forms (multi, per-tensor, capturable): after 3 steps
    the shadow is p.half() bit for bit and marked current, p.grad is zeros, the gaps of the
    flat buffer are untouched, and p / exp_avg / exp_avg_sq agree across the forms bit for
    bit."""
    from atmonr_amd.optim import FusedAdam

    shapes = [(1025,), (37, 5), (4097,), (3,)]
    rng = np.random.default_rng(21)
    p0 = [ar.workload_params(rng, int(np.prod(s))).reshape(s) for s in shapes]
    grads = [ar.workload_grads(rng, int(np.prod(s)), 3) for s in shapes]
    results = {}
    for form in ("multi", "per_tensor", "capturable"):
        ps = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(dev)) for x in p0]
        flat = torch.full((sum(x.size for x in p0) + 2 * len(p0) + 9,), 7.0,
                          dtype=torch.float16, device=dev)
        used = torch.zeros(flat.numel(), dtype=torch.bool)
        off = 1
        for q in ps:
            assert off % 2 == 1
            q._anr_shadow = flat[off:off + q.numel()].view(q.shape)
            assert q._anr_shadow.data_ptr() % 4 == 2
            used[off:off + q.numel()] = True
            off += q.numel() + (2 if q.numel() % 2 == 0 else 1)
            q.grad = torch.zeros_like(q)
        opt = FusedAdam([{"params": ps[:2], "weight_decay": 0.0},
                         {"params": ps[2:], "weight_decay": 1e-2, "lr": 3e-3}], lr=LR,
                        betas=(B1, B2), eps=EPS, zero_grad_in_step=True,
                        capturable=form == "capturable")
        opt.multi_tensor = form != "per_tensor"
        for k in range(3):
            for q, g in zip(ps, grads):
                q.grad.copy_(torch.from_numpy(g[k].reshape(q.shape)))
            opt.step()
        torch.cuda.synchronize()
        for q in ps:
            assert torch.equal(q._anr_shadow.view(torch.int16), q.detach().half().view(torch.int16))
            assert q._anr_shadow_ver == q._version
            assert not q.grad.view(torch.int32).any()
        assert (flat.cpu()[~used] == 7.0).all()
        results[form] = [(q.detach().cpu().numpy(), opt.state[q]["exp_avg"].cpu().numpy(),
                          opt.state[q]["exp_avg_sq"].cpu().numpy()) for q in ps]
    for form in ("per_tensor", "capturable"):
        for i, (x, y) in enumerate(zip(results["multi"], results[form])):
            for k, u, w in zip(("p", "exp_avg", "exp_avg_sq"), x, y):
                ar.assert_bits_equal(w, u, f"{form} against multi, tensor {i} {k}")
    # and the moments are Adam's: the emulation chained over the same three steps
    for i, (x, g) in enumerate(zip(results["multi"], grads)):
        p, m, v = p0[i].ravel(), np.zeros(p0[i].size, f32), np.zeros(p0[i].size, f32)
        lr, wd = (LR, 0.0) if i < 2 else (3e-3, 1e-2)
        for k in range(3):
            p, m, v, _ = _emulate((p, g[k], m, v), lr=lr, wd=wd, decoupled=True, step=k + 1)
        for k, u, w in zip(("p", "exp_avg", "exp_avg_sq"), x, (p, m, v)):
            ar.assert_bits_equal(u.ravel(), w, f"FusedAdam against the emulation, tensor {i} {k}")
