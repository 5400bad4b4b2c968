"""GPU: the polyphase filter bank kernel (sy11_iq_channelize) against the float64 restatement of tests/_pfb_ref.py and against the
shipped DDC, far into a capture, from an odd base, the chunk independence of ``ChannelizedCapture``, and a channelised scan against
scans of the bank's own rows.

The parity bar is the DDC's rule: per case 4x the error of the float32 emulation in _pfb_ref (same fold order, same FFT schedule,
same twiddle table, no fma) against the float64 reference on the same input, relative to max |y| over the (K, M) block.  Parity is
unpinned against the reference project (the feature has no counterpart there) and pinned against ``_ddc_ref`` through
tests/test_channelize_cpu.py."""
import numpy as np
import pytest
import torch

from tests import _ddc_ref as R
from tests import _pfb_ref as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FS_IN = 1.0e6


def _plan(K, r):
    from sy11.data.channelize import plan_channels
    return plan_channels(FS_IN, K, r)


def _capture(n, seed=0):
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) + 1j * g.standard_normal(n)).astype(np.complex64)


def _errors(got, x, plan, n0=0, m0=0, M=None):
    want = P.plan_ref(x, plan, n0, m0, M)
    emu = P.plan_ref(x, plan, n0, m0, M, f32=True)
    scale = np.abs(want).max()
    assert got.shape == want.shape and got.dtype == np.complex64
    return np.abs(emu - want).max() / scale, np.abs(got.astype(np.complex128) - want).max() / scale, want


def _check(name, got, x, plan, n0=0, m0=0, M=None):
    e_emu, e_gpu, want = _errors(got, x, plan, n0, m0, M)
    print(f"iq_channelize[{name}]: {want.shape} outputs, float32 emulation {e_emu:.3e}, kernel {e_gpu:.3e} (bar {4 * e_emu:.3e})")
    assert e_emu > 0 and e_gpu <= 4 * e_emu, (name, e_gpu, e_emu)
    return e_emu


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("K,r,n", [(2, 1, 4099), (2, 2, 4099), (4, 2, 6001), (8, 1, 8191), (16, 2, 20001), (64, 2, 40001), (64, 1, 70003)])
def test_kernel_matches_the_float64_reference_on_every_output(K, r, n):
    """The whole capture in one call: every output of every channel, both zero-extended ends included."""
    from sy11 import ops
    plan = _plan(K, r)
    x = _capture(n, K * 100 + r)
    M = plan.n_out(n)
    got = ops.iq_channelize(torch.from_numpy(x).to(DEV), plan, 0, 0, M)
    assert got.shape == (K, M) and got.is_contiguous()
    _check(f"K={K} oversample={r} n={n}", got.cpu().numpy(), x, plan)


def test_rows_match_the_shipped_ddc():
    """Rows k = 0, 1, 8, 15 of (16, 2, 20001) against ``ops.iq_resample`` with ``plan.ddc_plan(k)``: two kernels for one
    definition, so they differ by at most the sum of their bars."""
    from sy11 import ops
    plan = _plan(16, 2)
    n = 20001
    x = _capture(n, 1602)
    dev = torch.from_numpy(x).to(DEV)
    M = plan.n_out(n)
    got = ops.iq_channelize(dev, plan, 0, 0, M).cpu().numpy()
    e_pfb = _check("K=16 oversample=2 (DDC cross-check)", got, x, plan)
    for k in (0, 1, 8, 15):
        d = plan.ddc_plan(k)
        assert d.n_out(n) == M
        row = ops.iq_resample(dev, d, 0, 0, M).cpu().numpy()
        want = R.plan_ref(x, d)
        scale = np.abs(want).max()
        e_ddc = np.abs(R.plan_ref(x, d, f32=True) - want).max() / scale
        diff = np.abs(got[k].astype(np.complex128) - row.astype(np.complex128)).max() / scale
        print(f"iq_channelize row {k} vs iq_resample: {diff:.3e} (bars {4 * e_pfb:.3e} + {4 * e_ddc:.3e})")
        assert diff <= 4 * e_pfb + 4 * e_ddc, (k, diff)


@pytest.mark.parametrize("K", [16, 64])
def test_far_into_a_capture(K):
    """in[] = samples [n0, n0 + 4096) with n0 near 3e9, an odd sample; m0 = ceil((n0 + N) / D), so the block reads nothing left of
    in[]: the residue r = i mod K and the tap index must come from the absolute index."""
    from sy11 import ops
    plan = _plan(K, 2)
    n0, n = 3 * 10 ** 9 + 1, 4096
    m0 = -(-(n0 + plan.N) // plan.D)
    M = (n0 + n - 1 - plan.c) // plan.D - m0 + 1
    a, b = plan.support(m0, m0 + M)
    assert n0 <= a and b <= n0 + n and M > 20 and n0 % 2 == 1
    x = _capture(n, K)
    got = ops.iq_channelize(torch.from_numpy(x).to(DEV), plan, n0, m0, M, n_total=n0 + n + 12345)
    _check(f"K={K} at n0={n0}", got.cpu().numpy(), x, plan, n0, m0, M)


def test_odd_input_base_and_wrapper_checks():
    """The input starts at an odd sample of its allocation (8-byte, not 16-byte aligned): same outputs, bit for bit, as from an
    aligned copy; the wrapper's argument errors raise before anything is launched."""
    from sy11 import _lib, ops
    plan = _plan(8, 2)
    n = 6001
    x = _capture(n, 4)
    buf = torch.zeros(n + 1, dtype=torch.complex64, device=DEV)
    buf[1:] = torch.from_numpy(x).to(DEV)
    odd = buf[1:]
    assert odd.data_ptr() % 16 == 8
    M = plan.n_out(n)
    got = ops.iq_channelize(odd, plan, 0, 0, M)
    _check("K=8 odd base", got.cpu().numpy(), x, plan)
    assert torch.equal(got, ops.iq_channelize(torch.from_numpy(x).to(DEV), plan, 0, 0, M))
    a, b = plan.support(300, 700)
    inner = ops.iq_channelize(odd[a:b], plan, a, 300, 400, n_total=n)
    assert torch.equal(inner, got[:, 300:700])
    out = torch.full((plan.K, 400), 7.0, dtype=torch.complex64, device=DEV)
    assert ops.iq_channelize(odd[a:b], plan, a, 300, 400, out=out, n_total=n) is out and torch.equal(out, inner)
    untouched = out.clone()
    for bad in ((odd[a + 1:b], a + 1), (odd[a:b - 1], a)):
        with pytest.raises(_lib.Sy11Error, match="read samples"):
            ops.iq_channelize(bad[0], plan, bad[1], 300, 400, out=out, n_total=n)
    with pytest.raises(_lib.Sy11Error):
        ops.iq_channelize(odd, plan, 0, 0, M + 1)
    with pytest.raises(_lib.Sy11Error):
        ops.iq_channelize(odd[a:b], plan, a, 300, 400)                      # n0 != 0 without the capture's length
    with pytest.raises(_lib.Sy11Error, match="`out`"):
        ops.iq_channelize(odd[a:b], plan, a, 300, 400, out=out[:, :399], n_total=n)
    with pytest.raises(_lib.Sy11Error, match="`out`"):
        ops.iq_channelize(odd[a:b], plan, a, 300, 400, out=out.T.contiguous(), n_total=n)
    with pytest.raises(_lib.Sy11Error):
        ops.iq_channelize(odd.to(torch.complex128), plan, 0, 0, M)
    with pytest.raises(_lib.Sy11Error):
        ops.iq_channelize(odd[::2], plan, 0, 0, 10)
    assert torch.equal(out, untouched)                                      # nothing was launched


# ------------------------------------------------------------------------------------------------------------- chunks
@pytest.mark.parametrize("K,r", [(8, 2), (64, 1), (2, 2)])
def test_channelized_capture_is_bit_identical_for_every_chunking_and_source(tmp_path, K, r):
    from sy11 import ops
    from sy11.data.channelize import ChannelizedCapture
    from sy11.data.spectrogram import open_iq
    plan = _plan(K, r)
    n = 6000 * plan.D + 7
    x = _capture(n, 6)
    x.view(np.float32).tofile(tmp_path / "capture.cf32")
    dev = torch.from_numpy(x).to(DEV)
    M = plan.n_out(n)
    whole = ops.iq_channelize(dev, plan, 0, 0, M)
    for name, src in (("host array", open_iq(x)), ("memmap", open_iq(str(tmp_path / "capture.cf32"))), ("device tensor", open_iq(dev))):
        cap = ChannelizedCapture(src, plan, DEV)
        assert len(cap) == M
        for step in (1000, 4097, M):
            parts = [cap.block(lo, min(lo + step, M)) for lo in range(0, M, step)]
            assert all(p.is_cuda and p.dtype == torch.complex64 and p.shape[0] == K for p in parts)
            assert torch.equal(torch.cat(parts, 1), whole), (name, step)
        blk = cap.block(1500, 2601)
        assert cap.block(1500, 2601) is blk                                 # the last block is kept
        for k in (0, K // 2, K - 1):
            ch = cap.channel(k)
            assert ch.yields_device and len(ch) == M
            assert torch.equal(ch[1500:2601], blk[k])
            assert torch.equal(ch[17:1018], whole[k, 17:1018])              # another range: computed, then cached
        with pytest.raises(ValueError):
            cap.block(0, M + 1)
        with pytest.raises(ValueError):
            cap.channel(K)


# ------------------------------------------------------------------------------------------------------------- end to end
def _model(nc=2):
    from oracle import yolo11_ref as Y
    from sy11.nn.tasks import DetectionModel
    m = DetectionModel("yolo11n.yaml", nc=nc, verbose=False)
    sd = Y.seeded_state_dict(Y.empty_state_dict(Y.resolve_graph("n", nc=nc)), seed=7)
    for k in sd:                                               # confident random head, as tests/test_scan_gpu.py builds it
        if ".cv3." in k and k.endswith("2.bias"):
            sd[k] = sd[k] + 1.0
    m.load_state_dict(sd)
    m.names = {i: f"class_{i}" for i in range(nc)}
    return m


@pytest.fixture(scope="module")
def scanner():
    from sy11.data import spectrogram as sp
    from sy11.engine.predictor import DetectionPredictor
    from tests import _scan_ref as S
    pred = DetectionPredictor(_model(2), device=DEV, conf=0.05, iou=0.7, producer=sp.SpectrogramProducer(DEV))
    return pred, S.capture(6.2)                                             # at 2 fs_out: about three windows per band


@pytest.mark.parametrize("batch", [1, 64])
def test_channelised_scan_equals_scans_of_the_bank_rows(scanner, batch):
    from sy11.data import spectrogram as sp
    from sy11.data.channelize import ChannelizedCapture, merge_channels, plan_channels
    pred, x = scanner
    fs_in, fc = 40e6, 2.4e9
    plan = plan_channels(fs_in, 4, 2)
    fs = plan.fs_out
    assert fs == 20e6 and plan.default_select() == [0, 1, 3]
    rows = ChannelizedCapture(x.to(DEV), plan, DEV).block(0, plan.n_out(len(x)))
    src = sp.open_iq(x)
    got = pred.scan(src, fs_in, fc, channels=4, merge=None, batch=batch)
    assert got.channelizer.K == 4 and got.resample is None and got.sample_rate == fs and got.center_freq == fc
    assert got.channel.dtype == torch.int64 and got.channel.tolist() == sorted(got.channel.tolist())
    assert len(got.start) >= 3 and set(got.channel.tolist()) == {0, 1, 3}
    merged = []
    for k in (0, 1, 3):
        centre = fc + float(plan.offset_hz[k])
        want = pred.scan(sp.open_iq(rows[k]), fs, centre, merge=None, batch=batch)
        sel = got.channel == k
        assert len(want) > 0 and got.start.tolist() == want.start.tolist()
        for name in ("boxes", "window", "tf"):
            assert torch.equal(getattr(got, name)[sel], getattr(want, name)), (batch, k, name)
        assert want.channel is None and want.channelizer is None
        b = got.boxes[sel].numpy()
        assert torch.equal(got.tf[sel], torch.from_numpy(np.stack((sp.cols_to_time(b[:, 0] - 0.5, fs), sp.rows_to_freq(b[:, 1] - 0.5, fs, centre),
                                                                    sp.cols_to_time(b[:, 2] - 0.5, fs), sp.rows_to_freq(b[:, 3] - 0.5, fs, centre)), 1)))
        assert float(got.tf[sel][:, 1].min()) >= centre - fs / 2 - 1 and float(got.tf[sel][:, 3].max()) <= centre + fs / 2 + 1
        merged.append(pred.scan(sp.open_iq(rows[k]), fs, centre, merge="ios", batch=batch))
    assert float(got.tf[:, 2].max()) <= len(x) / fs_in                      # seconds of the capture
    # merge="ios": the per-band seam merges, then the cross-band merge in seconds / Hz
    boxes, window, tf = (torch.cat([getattr(m, name) for m in merged]) for name in ("boxes", "window", "tf"))
    chan = torch.cat([torch.full((len(m),), k, dtype=torch.int64) for k, m in zip((0, 1, 3), merged)])
    keep = torch.from_numpy(merge_channels(tf.numpy(), boxes[:, 4].numpy(), boxes[:, 5].numpy(), chan.numpy(), "ios", 0.5, False))
    both = pred.scan(src, fs_in, fc, channels=plan, merge="ios", batch=batch)
    assert 0 < len(both) <= len(boxes) < len(got)
    for name, want in (("boxes", boxes), ("window", window), ("tf", tf), ("channel", chan)):
        assert torch.equal(getattr(both, name), want[keep]), (batch, name)
    # oversample = 1: bands do not overlap, no cross-band merge; select picks bands
    one = pred.scan(src, fs_in, fc, channels=2, oversample=1, select=[0], merge="ios", batch=batch)
    assert one.channelizer.D == 2 and set(one.channel.tolist()) <= {0}
    want = pred.scan(sp.open_iq(ChannelizedCapture(x.to(DEV), one.channelizer, DEV).block(0, len(rows[0]))[0]), fs, fc, merge="ios", batch=batch)
    assert torch.equal(one.boxes, want.boxes) and torch.equal(one.tf, want.tf)


def test_scan_without_channels_is_unchanged(scanner):
    from sy11.data import spectrogram as sp
    pred, x = scanner
    y = x[:len(x) // 2]
    a = pred.scan(sp.open_iq(y), 20e6, 2.4e9, batch=64)
    b = pred.scan(sp.open_iq(y), 20e6, 2.4e9, batch=64, channels=None, oversample=2, select=None)
    assert len(a) > 0 and a.channel is None and a.channelizer is None
    for name in ("boxes", "window", "tf"):
        assert torch.equal(getattr(a, name), getattr(b, name))
