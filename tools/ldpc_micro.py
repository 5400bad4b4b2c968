"""Time the min-sum launch of the LDPC frame decoder (sy11_ldpc_decode: ONE launch over all frames, one workgroup per frame) on noisy codewords of a seeded
staircase code (sy11.data.ldpc.ldpc_staircase: mb x nb blocks of size Z, six information entries a row), BPSK over AWGN at --ebn0 dB, soft_scale 16.  Without
--force a frame stops at the first iteration that satisfies every check; with --force the soft bits are noise alone, no frame converges and every frame runs all
--iterations (the tool checks that it did).  Per workload one warm-up call, then REPS calls, each between two events on the stream; the median is printed.  A
call is the library's entry point with every table already on the device: its host-side checks and the kernel.  The first frames' bits, iteration counts and
posteriors are compared with the numpy definition's (tests/_ldpc_ref.py).  --viterbi adds the Viterbi launch of `decode` (sy11_fec_viterbi, as
tools/decode_micro.py times it) over as many frames of as many information bits, with a tail, for context.  The dynamic LDS of the code and the workgroups a
compute unit holds by it (160 KiB of LDS, 32 waves) are printed: computed, not measured.
Usage: ldpc_micro.py [--frames 4096] [--Z 81] [--mb 12] [--nb 24] [--iterations 20] [--scale 12] [--ebn0 3.0] [--force] [--viterbi] [--reps 10] [--check 8]
       ldpc_micro.py --suite        the three workloads DESIGN.md §6 records"""
import argparse
import ctypes as C
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import _lib
from sy11.data.decode import FECFRAME
from sy11.data.ldpc import ldpc_encode, ldpc_staircase
from tests import _ldpc_ref as R

dev = torch.device("cuda", 0)
p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731


def timed(name, args, reps):
    _lib.call(name, *args)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call(name, *args)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def run(frames, Z, mb, nb, iterations, scale, ebn0, force, viterbi, reps, check):
    cd = ldpc_staircase(nb - mb, mb, Z, 1, row_weight=min(6, nb - mb))
    n, N, K = frames, cd.N, cd.K
    g = np.random.default_rng(Z + frames)
    sigma = np.sqrt(1.0 / (2.0 * (K / N) * 10.0 ** (ebn0 / 10.0)))
    if force:
        y = np.clip(np.rint(16.0 * sigma * g.standard_normal((n, N))), -127, 127).astype(np.int8)
        c = None
    else:
        c = ldpc_encode(g.integers(0, 2, (n, K)), cd)
        y = np.clip(np.rint(16.0 * ((1.0 - 2.0 * c) + sigma * g.standard_normal((n, N)))), -127, 127).astype(np.int8)
    lds = int(_lib.load().sy11_ldpc_lds_bytes(Z, mb, nb, cd.entry.shape[0]))
    W = min(256, 64 * -(-Z // 64))
    per_cu = min(160 * 1024 // lds, 32 * 64 // W)
    row = np.arange(n, dtype=np.int32)
    host = np.concatenate((row, cd.layer, cd.entry.view(np.int32)))
    table = torch.from_numpy(host).to(dev)
    soft = torch.from_numpy(y).to(dev)
    bits = torch.zeros((n, (N + 7) // 8), dtype=torch.uint8, device=dev)
    out = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    post = torch.zeros((n, N), dtype=torch.int16, device=dev)
    spec = _lib.LdpcCode(cd.Z, cd.mb, cd.nb, cd.entry.shape[0])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (n, C.c_void_p(row.ctypes.data), p(table), C.byref(spec), C.c_void_p(cd.layer.ctypes.data), C.c_void_p(table.data_ptr() + 4 * n), C.c_void_p(cd.entry.ctypes.data),
            C.c_void_p(table.data_ptr() + 4 * (n + cd.layer.shape[0])), iterations, scale, n, N, p(soft), bits.shape[1], p(bits), p(out), N, p(post), stream)
    t, lo, hi = timed("sy11_ldpc_decode", args, reps)
    h = out.cpu().numpy()
    if force and not (h[:, 0] == iterations).all():
        raise SystemExit(f"--force: {int((h[:, 0] < iterations).sum())} frames stopped before iteration {iterations}")
    m = min(check, n)
    ref = R.decode(y[:m], cd.base, Z, iterations, scale)
    same = np.array_equal(np.unpackbits(bits[:m].cpu().numpy(), axis=1)[:, :N], ref["x"]) and np.array_equal(h[:m, 0], ref["iterations"]) and np.array_equal(h[:m, 1], ref["unsat"]) \
        and np.array_equal(post[:m].cpu().numpy(), ref["post"])
    sweeps = int(h[:, 0].sum())
    edges = cd.entry.shape[0] * Z
    decoded = "" if c is None else f", {int((np.unpackbits(bits.cpu().numpy(), axis=1)[:, :N] == c).all(axis=1).sum())} of {n} decoded as sent"
    print(f"  {n:5d} frames, {mb} x {nb}, Z = {Z} (N = {N}, K = {K}, {edges} edges), {'all ' + str(iterations) + ' iterations forced' if force else f'early stop at {ebn0} dB'}: "
          f"{t:8.3f} ms (min {lo:.3f}, max {hi:.3f}) = {t / n * 1e3:8.2f} us per frame, {sweeps / n:5.2f} iterations a frame, {sweeps * edges / t / 1e6:8.2f} G edge updates/s, "
          f"{n * K / t / 1e6:8.2f} Gbit/s of information{decoded};  LDS {lds} B, {W} threads: {per_cu} workgroups per CU (computed);  "
          f"the first {m} frames {'equal' if same else 'DIFFER FROM'} numpy's")
    if viterbi:
        T = min(K + 6, 8192)
        fr = np.zeros(n, dtype=FECFRAME)
        fr["T"], fr["order"], fr["tail"], fr["row"], fr["scale"] = T, 2, 1, np.arange(n), 1.0
        ftab = torch.from_numpy(fr.view(np.uint8)).to(dev)
        vsoft = torch.from_numpy(g.integers(-64, 65, (n, 2 * T)).astype(np.int8)).to(dev)
        vbits = torch.zeros((n, (T + 7) // 8), dtype=torch.uint8, device=dev)
        vout = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        vargs = (n, C.c_void_p(fr.ctypes.data), p(ftab), 0o171, 0o133, n, 2 * T, p(vsoft), vbits.shape[1], p(vbits), p(vout), stream)
        tv, vlo, vhi = timed("sy11_fec_viterbi", vargs, reps)
        print(f"        for context, the Viterbi launch over {n} frames of T = {T} ({T - 6} information bits): {tv:8.3f} ms (min {vlo:.3f}, max {vhi:.3f}) = {tv / n * 1e3:8.2f} us per frame, "
              f"{n * (T - 6) / tv / 1e6:8.2f} Gbit/s of information")
    return same


def main():
    a = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    a.add_argument("--frames", type=int, default=4096)
    a.add_argument("--Z", type=int, default=81)
    a.add_argument("--mb", type=int, default=12)
    a.add_argument("--nb", type=int, default=24)
    a.add_argument("--iterations", type=int, default=20)
    a.add_argument("--scale", type=int, default=12)
    a.add_argument("--ebn0", type=float, default=3.0)
    a.add_argument("--force", action="store_true")
    a.add_argument("--viterbi", action="store_true")
    a.add_argument("--reps", type=int, default=10)
    a.add_argument("--check", type=int, default=8)
    a.add_argument("--suite", action="store_true")
    o = a.parse_args()
    print(f"LDPC frame decoder, launch 2, {torch.cuda.get_device_name(0)}: scale {o.scale}/16, {o.reps} calls after one warm-up, the median")
    if o.suite:
        ok = run(4096, 81, 12, 24, 20, o.scale, 3.0, True, True, o.reps, o.check)
        ok &= run(4096, 81, 12, 24, 20, o.scale, 3.0, False, False, o.reps, o.check)
        ok &= run(256, 512, 16, 32, 20, o.scale, 3.0, True, True, o.reps, 1)
        ok &= run(256, 512, 16, 32, 20, o.scale, 3.0, False, False, o.reps, 1)
    else:
        ok = run(o.frames, o.Z, o.mb, o.nb, o.iterations, o.scale, o.ebn0, o.force, o.viterbi, o.reps, o.check)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
