"""Plain-torch CPU reference of the attention core of csrc/attention.hip (sy11_attention_fwd, sy11_attention_bwd[_o]), in parts:
one function per product or elementwise step, so that every quantity a kernel writes (P, o, the row sums, dq, dk, dv) has a
reference of its own.  Not a test module.

Every function takes tensors that are ALREADY rounded to the kernel's storage dtype (q, k, v, dO, o) or to f32 (P) and evaluates
the formula in the compute dtype ``dt``.  The parity tests call each once with torch.float64 (``r64``) and once with torch.float32
(``r32``); tests/_kernel_ref.py derives the bar from the difference of the two.  Per-head tensors are (B, heads, N, d).

    s = scale * q k^T          P = softmax_j(s)            o = P v
    dP = dO v^T                delta_i = sum_j dP_ij P_ij = sum_e dO_ie o_ie
    dS = P (dP - delta)        dq = scale * dS k           dk = scale * dS^T q          dv = P^T dO

``extras`` holds the terms the bar gets beyond 8 * e_ref + u * max|r64|: one per rounding the kernels are documented to make
("Attention parity").  Each is a function of the float64 reference and the inputs, never of a kernel's output.
"""
from collections import namedtuple

import torch

from tests._kernel_ref import HALF_ULP, rnd, rounded

F32, F64 = torch.float32, torch.float64
ATT_QT = 32
ATT_LDS_MAX = 160 * 1024


def kernel_scale(kd):
    """kd^-0.5 as the library takes it: 1.0f / sqrtf((float)kd), two correctly rounded f32 operations."""
    return float(torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(kd), dtype=F32)))


# ------------------------------------------------------------------------------------------------ inputs
REGIMES = ("flat", "peaked", "dominant_last", "dominant_first")
DOM_Q, DOM_K, DOM_V = 4.0, 256.0, 2.0 ** -8     # exact in f16 / bf16; scale * (4 * 256 - kd - 3) > 104 = -ln(smallest f32 denormal), kd <= 64


def inputs(B, heads, N, kd, hd, dtype, regime, seed=1):
    """-> qkv (B, N, heads * (2 kd + hd)), dO (B, N, heads * hd): CPU f32 holding values of the storage ``dtype``.

    flat      uniform in [-1, 1]: scores of about +-0.6, every P about 1 / N.
    peaked    q and k times 6 before rounding: scores with a standard deviation of 12, row maxima of P near 1, most of a row below
              f32's exp underflow relative to its maximum.
    dominant_last / dominant_first
              every query of a (image, head) pair gets q_0 = 4 and the last / first key becomes (256, 0, ..., 0): its score
              scale * 1024 exceeds every other (<= scale * (kd + 3)) by more than 104, so in f32 P is exactly one-hot.  With a
              one-hot P dS, dq and dk are identically zero, which would leave the backward's scale factors unobserved; so only the
              pairs with (image + head) even are dominant and the others keep their flat rows (both heads and both images carry one
              of each, a single (image, head) is dominant).  The dominant key's v row is scaled by 2^-8: o = v_dominant there, and
              with the row sums taken from a 16-bit o the allowance u * sum|dO o| * 256 for dq (see ``extras``; it is a maximum
              over elements) would otherwise exceed the gradients of the flat pairs and hide a wrong scale factor
              (tests/test_attention_ref_cpu.py: every mutant has to land over the bar in this regime too)."""
    assert regime in REGIMES, regime
    hc = 2 * kd + hd
    x = rnd(B, N, heads, hc, seed=seed)
    if regime == "peaked":
        x[..., :2 * kd] *= 6.0
    elif regime.startswith("dominant"):
        j = N - 1 if regime == "dominant_last" else 0
        for b in range(B):
            for h in range(heads):
                if (b + h) % 2 == 0:
                    x[b, :, h, 0] = DOM_Q
                    x[b, j, h, kd:2 * kd] = 0.0
                    x[b, j, h, kd] = DOM_K
                    x[b, j, h, 2 * kd:] *= DOM_V
    return rounded(x.reshape(B, N, heads * hc), dtype), rounded(rnd(B, N, heads * hd, seed=seed + 1), dtype)


def is_dominant(b, h):
    return (b + h) % 2 == 0


# ------------------------------------------------------------------------------------------------ layout
def split_heads(qkv, heads, kd, hd):
    """(B, ..., heads * (2 kd + hd)) pixels, per head the channels [q(kd) | k(kd) | v(hd)] -> q, k (B, heads, N, kd), v (B, heads, N, hd)"""
    B, hc = qkv.shape[0], 2 * kd + hd
    assert qkv.shape[-1] == heads * hc, (tuple(qkv.shape), heads, kd, hd)
    x = qkv.reshape(B, -1, heads, hc).permute(0, 2, 1, 3)
    return x[..., :kd], x[..., kd:2 * kd], x[..., 2 * kd:]


def merge_heads(q, k, v):
    """Inverse of split_heads: -> (B, N, heads * (2 kd + hd))"""
    x = torch.cat((q, k, v), -1)
    B, heads, N, hc = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, heads * hc)


def split_o(o, heads, hd):
    """(B, ..., heads * hd) -> (B, heads, N, hd)"""
    return o.reshape(o.shape[0], -1, heads, hd).permute(0, 2, 1, 3)


def merge_o(o):
    B, heads, N, hd = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, N, heads * hd)


# ------------------------------------------------------------------------------------------------ forward, in parts
def scores(q, k, scale, dt=F64):
    return (q.to(dt) @ k.to(dt).transpose(-2, -1)) * scale


def softmax_rows(s):
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    return e / e.sum(-1, keepdim=True)


def out(P, v, dt=F64):
    return P.to(dt) @ v.to(dt)


# ------------------------------------------------------------------------------------------------ backward, in parts
def dP(dO, v, dt=F64):
    return dO.to(dt) @ v.to(dt).transpose(-2, -1)


def delta_from_P(dP_, P, dt=F64):
    return (dP_.to(dt) * P.to(dt)).sum(-1)


def delta_from_o(dO, o, dt=F64):
    return (dO.to(dt) * o.to(dt)).sum(-1)


def dS(P, dP_, delta, dt=F64):
    return P.to(dt) * (dP_.to(dt) - delta.to(dt).unsqueeze(-1))


def dq(dS_, k, scale, dt=F64):
    return (dS_.to(dt) @ k.to(dt)) * scale


def dk(dS_, q, scale, dt=F64):
    return (dS_.to(dt).transpose(-2, -1) @ q.to(dt)) * scale


def dv(P, dO, dt=F64):
    return P.to(dt).transpose(-2, -1) @ dO.to(dt)


def forward(q, k, v, scale, dt=F64):
    """-> dict s, P, o"""
    s = scores(q, k, scale, dt)
    P = softmax_rows(s)
    return dict(s=s, P=P, o=out(P, v, dt))


def backward(q, k, v, dO, P, scale, dt=F64, o=None):
    """The backward from a GIVEN P (f32 storage, as the kernels read it).  ``o`` given: the row sums are dO . o (what the MFMA path does
    with the forward output at hand), else sum_j dP P.  -> dict P_in (the P given), dP, delta, dS, dq, dk, dv"""
    dP_ = dP(dO, v, dt)
    delta = delta_from_P(dP_, P, dt) if o is None else delta_from_o(dO, o, dt)
    dS_ = dS(P, dP_, delta, dt)
    return dict(P_in=P, dP=dP_, delta=delta, dS=dS_, dq=dq(dS_, k, scale, dt), dk=dk(dS_, q, scale, dt), dv=dv(P, dO, dt))


Reference = namedtuple("Reference", "q k v dO scale f64 f32 P_in o_in b64 b32 delta_o64 delta_o32")


def reference(qkv, dO, heads, kd, hd, dtype, scale=None):
    """Everything the parity tests compare against, from storage-rounded qkv / dO.  The backward references start from ``P_in`` (the
    float64 P rounded to f32, what the tests hand the backward kernels) and, for the row sums taken from the forward output, from
    ``o_in`` (the float64 o rounded to ``dtype``): a backward kernel's error is then its own."""
    scale = kernel_scale(kd) if scale is None else scale
    q, k, v = split_heads(qkv, heads, kd, hd)
    do = split_o(dO, heads, hd)
    f64, f32 = forward(q, k, v, scale, F64), forward(q, k, v, scale, F32)
    P_in = f64["P"].to(F32)
    o_in = f64["o"].to(dtype).to(F32)
    return Reference(q, k, v, do, scale, f64, f32, P_in, o_in, backward(q, k, v, do, P_in, scale, F64), backward(q, k, v, do, P_in, scale, F32),
                     delta_from_o(do, o_in, F64), delta_from_o(do, o_in, F32))


# ------------------------------------------------------------------------------------------------ dispatch
Path = namedtuple("Path", "fwd bwd delta_from_o")


def expected_path(dtype, N, kd, hd, lds, ptr_offsets, have_o):
    """The dispatch rule of sy11_attention_fwd / sy11_attention_bwd_o (csrc/attention.hip), restated.

    ``lds``: pixel strides in elements, keys qkv, o, do, dqkv.  ``ptr_offsets``: byte offsets of the base pointers from a 16-byte boundary,
    same keys plus p (missing keys count as 0).  ``have_o``: the forward output is passed to the backward.
    -> Path(fwd, bwd, delta_from_o): each direction one of "mma", "fast", "generic", "gs"; delta_from_o says whether the backward takes the
    row sums from o (MFMA path, o given, o's stride a multiple of 8 elements and its pointer 16-byte aligned)."""
    off = lambda name: ptr_offsets.get(name, 0) % 16                                   # noqa: E731
    head_ok = dtype != F32 and kd == 32 and hd == 64 and N % 4 == 0 and N >= 32
    fwd_mma = head_ok and lds["qkv"] % 8 == 0 and lds["o"] % 8 == 0 and off("qkv") == 0 and off("o") == 0 and off("p") == 0
    bwd_mma = (head_ok and lds["qkv"] % 8 == 0 and lds["do"] % 8 == 0 and off("qkv") == 0 and off("do") == 0
               and lds["dqkv"] % 8 == 0 and off("dqkv") == 0 and off("p") == 0 and -(-N // 32) * 32 * 64 <= 150 * 1024)

    def valu(fast_bytes, generic_bytes):
        if fast_bytes > ATT_LDS_MAX or generic_bytes > ATT_LDS_MAX:
            return "gs"
        return "fast" if (kd, hd) == (32, 64) else "generic"

    fwd = "mma" if fwd_mma else valu((ATT_QT * N + ATT_QT * 32 + 64 * 64) * 4, (ATT_QT * N + ATT_QT * kd + 64 * (kd + 1)) * 4)
    bwd = "mma" if bwd_mma else valu((ATT_QT * N + ATT_QT * 64 + 64 * 65) * 4, (ATT_QT * N + ATT_QT * hd) * 4)
    return Path(fwd, bwd, bool(bwd_mma and have_o and lds["o"] % 8 == 0 and off("o") == 0))


def supported(kd, hd):
    """Head sizes the library takes (att_check): anything else is SY11_ERR_* and leaves the outputs alone."""
    return 0 < kd <= 64 and 0 < hd <= 128 and 32 * (kd + hd) <= 16 * 256


# ------------------------------------------------------------------------------------------------ the bar's extra terms
def extras(path, dtype, fw, bw, q, k, v, dO, scale, o_in=None, o_err=None):
    """Allowances beyond 8 * e_ref + u * max|r64|, one per DOCUMENTED rounding, each the max over elements of a first-order bound.

    ``fw`` / ``bw``: the float64 dicts of forward() / backward().  u = half an ulp of the 16-bit type.
      P   (all paths)  2^-22 * P |s - rowmax|: the fast exponent evaluates 2^(x log2 e); rounding the f32 argument x log2 e (<= 2^-24
                       relative, x up to ~100) moves the result by P * |x| * 2^-24 relative to 1 — twice (the product and the reduced
                       argument of the hardware exp2), hence 2^-22 with a factor 2 to spare.  Zero for a flat softmax.
      MFMA path only (f16 / bf16; the VALU kernels keep every intermediate in f32):
      o   u * P |v|            P is rounded to 16 bit before P v      (each P_ij moves by <= u P_ij)
      dv  u * P^T |dO|         the same rounded P in P^T dO
      dq  u * scale |dS| |k|   dS is rounded to 16 bit before dS k
      dk  u * scale |dS|^T |q|
      with the row sums from o (``o_in``, the 16-bit forward output) additionally, for dq and dk: delta_i moves by
          dd_i = sum_e |dO_ie| * |error of o_ie|,   error of o_ie <= u |o_ie| for an o that is the exact product rounded once
          (``o_err`` overrides that per-element bound: the end-to-end cases pass the forward's own bar),
          dS_ij by P_ij dd_i, so dq by scale * dd_i (P |k|)_id and dk by scale * ((P dd)^T |q|)_jd.
    -> dict name -> float for P, o, dq, dk, dv (missing = 0)."""
    d = F64
    ex = {}
    if fw is not None:
        s, P = fw["s"], fw["P"]
        ex["P"] = 2.0 ** -22 * float((P * (s - s.max(-1, keepdim=True).values).abs()).max())
        if path.fwd == "mma":
            ex["o"] = HALF_ULP[dtype] * float((P @ v.to(d).abs()).max())
    if bw is not None and path.bwd == "mma":
        u = HALF_ULP[dtype]
        P, dS_ = bw["P_in"].to(d), bw["dS"]
        ex["dv"] = u * float((P.transpose(-2, -1) @ dO.to(d).abs()).max())
        ex["dq"] = u * scale * float((dS_.abs() @ k.to(d).abs()).max())
        ex["dk"] = u * scale * float((dS_.abs().transpose(-2, -1) @ q.to(d).abs()).max())
        if path.delta_from_o:
            oe = u * o_in.to(d).abs() if o_err is None else torch.full_like(o_in.to(d), float(o_err))
            dd = (dO.to(d).abs() * oe).sum(-1, keepdim=True)
            ex["dq"] += scale * float((dd * (P @ k.to(d).abs())).max())
            ex["dk"] += scale * float(((P * dd).transpose(-2, -1) @ q.to(d).abs()).max())
    return ex
