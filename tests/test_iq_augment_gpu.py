"""GPU: sy11_iq_gather_augment against the float64 restatement (tests/_iq_ref.py).

Error measure: max |out - ref| / max |ref| (noise: relative to sigma).  BAR comes from the float32 floor of the restatement, not
from the device: per source the angle is rounded twice (int32 -> float and the product with pi 2^-31: <= 3.7e-7 rad), sincosf and
the three roundings of the rotation and the gain add ~ 4e-7, all relative to |z| <= max |ref|; a noise sample carries the same
angle error times its radius (<= 3.2 over 4 864 samples) plus logf / sqrtf: <= 2e-6 of sigma in the worst case.  The same float32
arithmetic evaluated on the host (the kernel's body compiled as plain C++ with glibc's sinf / cosf / logf) gives 1.7e-7 (shift),
1.9e-7 (conjugate + shift), 2.3e-7 (everything), 2.0e-7 (164 608 samples, 82 000 wraps) and 5.3e-7 of sigma (noise only); BAR is
4 x the largest of these.  The float64-vs-MI355X figures have NOT been measured yet (no device was available when this was
written): every case prints its figure, and once they are recorded in DESIGN.md §5 the bar becomes 4 x the measured maximum; a
measured value above 1e-5 is a finding to explain, not to accommodate."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _iq_ref as R

pytestmark = pytest.mark.gpu

BAR = 4 * 5.3e-7
L = 4864                                                     # 16 frames of 1024 / 256
OFFS = (0, 1, 4097)                                          # even, odd, odd and past a page


@pytest.fixture(scope="module")
def sources():
    """Three captures at distinct base pointers plus a partner buffer, on the host (complex64) and on the device."""
    rng = np.random.default_rng(2024)
    host = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) for n in (L, L + 1, L + 4097, L + 333)]
    dev = [torch.from_numpy(h).cuda() for h in host]
    assert len({d.data_ptr() for d in dev}) == 4
    return host, dev


def run(sources, mix=False, **fields):
    """Launch B = 3 with the same recipe fields in every row -> (device output as complex64 numpy, float64 reference)."""
    from sy11 import _lib, ops
    host, dev = sources
    rec = ops.iq_recipes(3)
    flags = (_lib.IQ_CONJ if fields.pop("conj", False) else 0) | (_lib.IQ_CONJ2 if fields.pop("conj2", False) else 0)
    for k, v in fields.items():
        rec[k] = v
    rec["flags"] = flags
    if mix:
        rec["off2"] = 333                                                     # the partner: a fourth buffer at an odd offset
    out = ops.iq_gather_augment(dev[:3], OFFS, L, rec, [dev[3]] * 3 if mix else None)
    torch.cuda.synchronize()
    ref = np.stack([R.gather_augment(host[b], OFFS[b], L, dphi=int(rec["dphi"][b]), phi0=int(rec["phi0"][b]), conj=bool(flags & 1),
                                     gain=float(rec["gain"][b]), src2=host[3] if mix else None, off2=333, dphi2=int(rec["dphi2"][b]),
                                     phi02=int(rec["phi02"][b]), conj2=bool(flags & 2), gain2=float(rec["gain2"][b]),
                                     sigma=float(rec["sigma"][b]), seed=int(rec["seed"][b])) for b in range(3)])
    return out.cpu().numpy(), ref


def rel_err(out, ref, scale=None):
    return float(np.abs(out.astype(np.complex128) - ref).max() / (scale if scale is not None else np.abs(ref).max()))


def test_identity_is_bit_exact(sources):
    from sy11 import ops
    host, dev = sources
    out = ops.iq_gather_augment(dev[:3], OFFS, L)
    want = torch.from_numpy(np.stack([host[b][OFFS[b]:OFFS[b] + L] for b in range(3)])).cuda()
    assert torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(want).view(torch.int32))


CASES = {
    "shift": dict(dphi=0x0A3D70A4, phi0=0x9E3779B9),
    "conj_shift": dict(conj=True, dphi=0xF0000001, phi0=0x12345678),
    "gain": dict(gain=10 ** (-4.5 / 20)),
    "mix": dict(mix=True, gain2=0.7, dphi2=0x40000000, phi02=0x80000000, conj2=True),
    "everything": dict(mix=True, conj=True, dphi=0x0A3D70A4, phi0=0x9E3779B9, gain=1.7, gain2=0.6, dphi2=0xC0000123, phi02=7,
                       sigma=0.8, seed=0xDEADBEEFCAFEF00D),
}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_against_float64(sources, name):
    out, ref = run(sources, **dict(CASES[name]))
    e = rel_err(out, ref)
    print(f"iq_gather_augment[{name}]: max |out - ref| / max |ref| = {e:.3e}  (bar {BAR:.3e})")
    assert e <= BAR


def test_noise_only_and_launch_shape_independence():
    from sy11 import ops
    zero = torch.zeros(L, dtype=torch.complex64, device="cuda")
    rec = ops.iq_recipes(1)
    rec["sigma"], rec["seed"] = 2.5, 0x0123456789ABCDEF
    out = ops.iq_gather_augment([zero], [0], L, rec).cpu().numpy()[0]
    ref = float(np.float32(2.5)) * R.noise(0x0123456789ABCDEF, L)
    e = rel_err(out, ref, scale=2.5)
    print(f"iq_gather_augment[noise]: max |out - ref| / sigma = {e:.3e}  (bar {BAR:.3e})")
    assert e <= BAR
    short = ops.iq_gather_augment([zero], [0], 256, rec).cpu().numpy()[0]
    assert np.array_equal(short[100:200].view(np.int32), out[100:200].view(np.int32))      # (seed, n) only, not the launch shape
    odd = ops.iq_gather_augment([zero], [1], 255, rec).cpu().numpy()[0]                     # odd L, odd offset: same samples again
    assert np.array_equal(odd[100:200].view(np.int32), out[100:200].view(np.int32))


def test_long_window_phase_wraps_exactly():
    """B = 1, L = 164 608 (the 640-frame window), dphi one step short of half a cycle: n dphi wraps ~ 82 000 times."""
    from sy11 import ops
    n = 164608
    rng = np.random.default_rng(5)
    host = (rng.standard_normal(n + 1) + 1j * rng.standard_normal(n + 1)).astype(np.complex64)
    rec = ops.iq_recipes(1)
    rec["dphi"], rec["phi0"] = 0x7FFFFFFF, 0xFFFFFFF0
    out = ops.iq_gather_augment([torch.from_numpy(host).cuda()], [1], n, rec).cpu().numpy()[0]
    ref = R.gather_augment(host, 1, n, dphi=0x7FFFFFFF, phi0=0xFFFFFFF0)
    e = rel_err(out, ref)
    tail = rel_err(out[-4096:], ref[-4096:])
    print(f"iq_gather_augment[long]: max err = {e:.3e}, over the last 4096 samples = {tail:.3e}  (bar {BAR:.3e})")
    assert e <= BAR


@pytest.mark.parametrize("k", [-37, 300])
def test_tone_moves_by_the_shift(k):
    from sy11 import _lib, ops
    n = 4096
    tone = torch.exp(2j * torch.pi * 100 / 1024 * torch.arange(n + 1, dtype=torch.float64)).to(torch.complex64).cuda()
    for conj, want in ((False, (100 + k) % 1024), (True, (-100 + k) % 1024)):
        rec = ops.iq_recipes(1)
        rec["dphi"] = (k * 2 ** 32 // 1024) & 0xFFFFFFFF
        rec["flags"] = _lib.IQ_CONJ if conj else 0
        out = ops.iq_gather_augment([tone], [0], n, rec)[0]
        peak = int(torch.fft.fft(out[:1024]).abs().argmax())
        assert peak == want, (k, conj, peak, want)


def test_guards_refuse_before_any_launch():
    from sy11 import _lib, ops
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.complex64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args, word in (((1, 8, None, p, p, p, s), b"null"), ((1, 0, p, p, p, p, s), b"positive"), ((1, -3, p, p, p, p, s), b"positive"),
                       ((40000, 65536, p, p, p, p, s), b"int32")):
        rc = lib.sy11_iq_gather_augment(*args)
        assert rc < 0 and word in lib.sy11_last_error(), (args[:2], rc, lib.sy11_last_error())
    with pytest.raises(_lib.Sy11Error, match="leave the capture"):
        ops.iq_gather_augment([buf], [1], 64)                                   # the wrapper checks the window against its capture
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.zeros_like(buf))
