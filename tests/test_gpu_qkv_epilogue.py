"""GPU: the qkv epilogue of RoPE + KV append (lade_rope_kv_append_ex / lade_rope_kv_append_parts_ex) against a torch restatement of
HF's Qwen2 / Qwen3 sequence in the model dtype:
  Qwen2   q / k / v = F.linear(h, W, b): the bias joins the fp32 sum before its one rounding (partials) - or, on a materialised qkv,
          one more rounding of (qkv + b);
  Qwen3   Qwen3RMSNorm over each q / k head (fp32 mean of squares, y = round(x * rsqrt(var + eps)), z = round(w * y)), then RoPE.
Bias only: bit-identical.  Head norm: the order of the sum of squares differs from torch's reduction, so y = round(x * rsqrt(var + eps))
may differ by one unit in the last place, and z = round(w * y) by two in 16-bit (checked directly at position 0, where RoPE is the
identity); after RoPE an element stays within two units in the last place of its operands (|z| of its pair), and nearly all are
bit-identical.  fp32 has no storage rounding to absorb
the difference between torch's rsqrt and the device's: 4 units on z, 8 after RoPE.  A null epilogue: bit-identical
to the plain entry points.  q, the K rows and the V^T columns written are checked, and nothing outside them is touched."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def _head_norm(x, w):
    """Qwen3RMSNorm (transformers/models/qwen3/modeling_qwen3.py) on [..., d] in the model dtype"""
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    return w * (xf * torch.rsqrt(var + EPS)).to(x.dtype)


def _reference(x_rows, H, Hkv, d, pos, cos, sin, bias, qn, kn, dtype):
    """x_rows [T, (H+2Hkv)d] = the rounded projection (bias included).  Returns (q [T,H,d], k [T,Hkv,d], v [T,Hkv,d], zq, zk): rotated q / k and
    the RoPE operands"""
    T = x_rows.shape[0]
    q = x_rows[:, :H * d].view(T, H, d)
    k = x_rows[:, H * d:(H + Hkv) * d].view(T, Hkv, d)
    v = x_rows[:, (H + Hkv) * d:].view(T, Hkv, d)
    if qn is not None:
        q = _head_norm(q, qn)
    if kn is not None:
        k = _head_norm(k, kn)
    c, s = cos[pos.long()][:, None], sin[pos.long()][:, None]
    return (q * c) + (_rotate_half(q) * s), (k * c) + (_rotate_half(k) * s), v, q, k


def _ulp(m, dtype):
    return torch.finfo(dtype).eps * torch.exp2(torch.floor(torch.log2(m.float().abs().clamp_min(1e-30))))


# units in the last place allowed for the head norm: on z itself and after RoPE (of its operands).  y = round(x * rsqrt(var + eps)) may
# land one unit away; z = round(w * y) scales that unit by |w| (1 + N(0, 0.2) here), so z may land two away.  In fp32 no rounding to the
# storage type absorbs the difference between torch's rsqrt and the device's, so the bounds are wider there.
ULPS_Z = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
ULPS_ROPE = {torch.float32: 8, torch.bfloat16: 2, torch.float16: 2}


def _ulp_bound(z, dtype):
    """ULPS_ROPE units in the last place of the larger RoPE operand of each pair (i, i + d/2)"""
    h = z.shape[-1] // 2
    m = torch.maximum(z[..., :h].float().abs(), z[..., h:].float().abs())
    return ULPS_ROPE[dtype] * _ulp(torch.cat((m, m), dim=-1), dtype) * 1.0001


def _check(got, ref, z, dtype, exact, what):
    if exact:
        assert torch.equal(got.float(), ref.float()), (what, (got.float() - ref.float()).abs().max().item())
        return
    diff = (got.float() - ref.float()).abs()
    bound = _ulp_bound(z, dtype)
    assert bool((diff <= bound).all()), (what, diff.max().item(), int((diff > bound).sum()))
    if dtype != torch.float32:
        assert float((diff == 0).float().mean()) >= 0.99, (what, "bit-identical share", float((diff == 0).float().mean()))


def _inputs(H, Hkv, d, T, dtype, epi, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    row_w = (H + 2 * Hkv) * d
    bias = (torch.randn(row_w, device="cuda", generator=g) * 0.5).to(dtype) if epi in ("bias", "both") else None
    qn = (1 + 0.2 * torch.randn(d, device="cuda", generator=g)).to(dtype) if epi in ("norm", "both") else None
    kn = (1 + 0.2 * torch.randn(d, device="cuda", generator=g)).to(dtype) if epi in ("norm", "both") else None
    rnd = random.Random(seed)
    pos = torch.tensor([rnd.randrange(4000) for _ in range(T)], dtype=torch.int32, device="cuda")
    return g, bias, qn, kn, pos


def _caches(Hkv, d, S_max, dtype):
    kc = torch.full((Hkv, S_max, d), float("nan"), dtype=dtype, device="cuda")
    vt = torch.full((Hkv, d, S_max), float("nan"), dtype=dtype, device="cuda")
    return kc, vt


CASES = [(H, Hkv, d) for d in (64, 128) for (H, Hkv) in ((2, 2), (12, 2), (14, 2))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,Hkv,d", CASES + [(4, 2, 12), (3, 1, 8)])           # (+ d = 12 / 8: the kernel's scalar path in fp32 / 16-bit)
@pytest.mark.parametrize("epi", ["bias", "norm", "both", "none"])
def test_materialised_qkv(dtype, H, Hkv, d, epi):
    from lookaheaddecoding_amd import ops
    from lookaheaddecoding_amd.engine import rope_tables
    T, P, S_max = 70, 5, 192
    dyn = d == 128 and H == 12
    g, bias, qn, kn, pos = _inputs(H, Hkv, d, T, dtype, epi, seed=H * 1000 + d)
    qkv = torch.randn(T, (H + 2 * Hkv) * d, device="cuda", generator=g).to(dtype)
    cos, sin = rope_tables(d, 4096, 1000000.0, dtype, "cuda")
    kc, vt = _caches(Hkv, d, S_max, dtype)
    dyn_P = torch.tensor([P], dtype=torch.int32, device="cuda") if dyn else None
    x, orig = qkv.clone(), qkv.clone()
    if epi == "none":
        q_old, kc_old, vt_old = qkv.clone(), kc.clone(), vt.clone()
        ops.rope_kv_append(q_old, pos, cos, sin, kc_old, vt_old, 0 if dyn else P, H=H, Hkv=Hkv, d=d, dyn_P=dyn_P)
        for e in (None, ops.qkv_epilogue(None, None, None, EPS)):
            q_new, kc_new, vt_new = qkv.clone(), kc.clone(), vt.clone()
            ops.rope_kv_append_ex(q_new, pos, cos, sin, kc_new, vt_new, 0 if dyn else P, H=H, Hkv=Hkv, d=d, dyn_P=dyn_P, epi=e)
            torch.cuda.synchronize()
            for a, b in ((q_new, q_old), (kc_new, kc_old), (vt_new, vt_old)):
                assert torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))
        return
    ops.rope_kv_append_ex(qkv, pos, cos, sin, kc, vt, 0 if dyn else P, H=H, Hkv=Hkv, d=d, dyn_P=dyn_P, epi=ops.qkv_epilogue(bias, qn, kn, EPS))
    torch.cuda.synchronize()
    if bias is not None:
        x = x + bias                                     # one rounding of (rounded projection + bias)
    rq, rk, v, zq, zk = _reference(x, H, Hkv, d, pos, cos, sin, bias, qn, kn, dtype)
    exact = epi == "bias"
    tag = (dtype, H, Hkv, d, epi)
    _check(qkv[:, :H * d].view(T, H, d), rq, zq, dtype, exact, ("q", tag))
    _check(kc[:, P:P + T].transpose(0, 1), rk, zk, dtype, exact, ("K rows", tag))
    assert torch.equal(vt[:, :, P:P + T].permute(2, 0, 1).float(), v.float()), ("V^T", tag)
    assert torch.equal(qkv[:, H * d:].float(), orig[:, H * d:].float()), tag          # (the k / v columns of qkv are left as they were)
    assert bool(torch.isnan(kc[:, :P].float()).all() and torch.isnan(kc[:, P + T:].float()).all()), tag
    assert bool(torch.isnan(vt[:, :, :P].float()).all() and torch.isnan(vt[:, :, P + T:].float()).all()), tag


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,Hkv,d", CASES)
@pytest.mark.parametrize("n_parts", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("epi", ["bias", "norm", "both", "none"])
def test_partials(dtype, H, Hkv, d, n_parts, epi):
    from lookaheaddecoding_amd import ops
    from lookaheaddecoding_amd.engine import rope_tables
    T, P, S_max = 60, 9, 128
    dyn = n_parts == 3
    g, bias, qn, kn, pos = _inputs(H, Hkv, d, T, dtype, epi, seed=n_parts * 100 + H + d)
    row_w = (H + 2 * Hkv) * d
    parts = torch.randn(n_parts, T, row_w, device="cuda", generator=g) * (1.0 / math.sqrt(n_parts))
    cos, sin = rope_tables(d, 4096, 1000000.0, dtype, "cuda")
    dyn_P = torch.tensor([P], dtype=torch.int32, device="cuda") if dyn else None
    Pa = 0 if dyn else P
    if epi == "none":
        q_old = torch.empty(T, H * d, dtype=dtype, device="cuda")
        kc_old, vt_old = _caches(Hkv, d, S_max, dtype)
        ops.rope_kv_append_parts(parts, n_parts, q_old, pos, cos, sin, kc_old, vt_old, T, Pa, H=H, Hkv=Hkv, d=d, dyn_P=dyn_P)
        for e in (None, ops.qkv_epilogue(None, None, None, EPS)):
            q_new = torch.empty(T, H * d, dtype=dtype, device="cuda")
            kc_new, vt_new = _caches(Hkv, d, S_max, dtype)
            ops.rope_kv_append_parts_ex(parts, n_parts, q_new, pos, cos, sin, kc_new, vt_new, T, Pa, H=H, Hkv=Hkv, d=d, dyn_P=dyn_P, epi=e)
            torch.cuda.synchronize()
            for a, b in ((q_new, q_old), (kc_new, kc_old), (vt_new, vt_old)):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        return
    q = torch.empty(T, H * d, dtype=dtype, device="cuda")
    kc, vt = _caches(Hkv, d, S_max, dtype)
    ops.rope_kv_append_parts_ex(parts, n_parts, q, pos, cos, sin, kc, vt, T, Pa, H=H, Hkv=Hkv, d=d, dyn_P=dyn_P,
                                epi=ops.qkv_epilogue(bias, qn, kn, EPS))
    torch.cuda.synchronize()
    acc = torch.zeros(T, row_w, device="cuda")
    for j in range(n_parts):                               # the partials in index order, then the bias, then one rounding
        acc = acc + parts[j]
    if bias is not None:
        acc = acc + bias.float()
    x = acc.to(dtype)
    rq, rk, v, zq, zk = _reference(x, H, Hkv, d, pos, cos, sin, bias, qn, kn, dtype)
    exact = epi == "bias"
    tag = (dtype, H, Hkv, d, n_parts, epi)
    _check(q.view(T, H, d), rq, zq, dtype, exact, ("q", tag))
    _check(kc[:, P:P + T].transpose(0, 1), rk, zk, dtype, exact, ("K rows", tag))
    assert torch.equal(vt[:, :, P:P + T].permute(2, 0, 1).float(), v.float()), ("V^T", tag)
    assert bool(torch.isnan(kc[:, :P].float()).all() and torch.isnan(kc[:, P + T:].float()).all()), tag
    assert bool(torch.isnan(vt[:, :, :P].float()).all() and torch.isnan(vt[:, :, P + T:].float()).all()), tag


def test_device_cache_length_past_the_cache_writes_nothing():
    """dyn_P + T > S_max (a hipGraph step replayed past its cache): the epilogue form returns without writing, as the plain one does"""
    from lookaheaddecoding_amd import ops
    from lookaheaddecoding_amd.engine import rope_tables
    dtype, H, Hkv, d, T, S_max = torch.bfloat16, 4, 2, 128, 8, 64
    g, bias, qn, kn, pos = _inputs(H, Hkv, d, T, dtype, "both", seed=5)
    parts = torch.randn(2, T, (H + 2 * Hkv) * d, device="cuda", generator=g)
    cos, sin = rope_tables(d, 4096, 10000.0, dtype, "cuda")
    kc, vt = _caches(Hkv, d, S_max, dtype)
    q = torch.full((T, H * d), float("nan"), dtype=dtype, device="cuda")
    dyn_P = torch.tensor([S_max - T + 1], dtype=torch.int32, device="cuda")
    ops.rope_kv_append_parts_ex(parts, 2, q, pos, cos, sin, kc, vt, T, 0, H=H, Hkv=Hkv, d=d, dyn_P=dyn_P, epi=ops.qkv_epilogue(bias, qn, kn, EPS))
    torch.cuda.synchronize()
    assert bool(torch.isnan(kc.float()).all() and torch.isnan(vt.float()).all() and torch.isnan(q.float()).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,Hkv,d", [(2, 2, 64), (14, 2, 64), (12, 2, 128), (7, 1, 128)])
@pytest.mark.parametrize("path", ["qkv", "parts"])
def test_head_norm_within_one_ulp(dtype, H, Hkv, d, path):
    """at position 0 (cos 1, sin 0) RoPE leaves z as it is: the kernel's normed q / k heads against HF's, element by element"""
    from lookaheaddecoding_amd import ops
    from lookaheaddecoding_amd.engine import rope_tables
    if path == "parts" and dtype == torch.float32:
        pytest.skip("the partials path is 16-bit only")
    T, S_max = 40, 64
    g, bias, qn, kn, _pos = _inputs(H, Hkv, d, T, dtype, "both", seed=H + d)
    pos = torch.zeros(T, dtype=torch.int32, device="cuda")
    cos, sin = rope_tables(d, 64, 10000.0, dtype, "cuda")
    kc, vt = _caches(Hkv, d, S_max, dtype)
    row_w = (H + 2 * Hkv) * d
    epi = ops.qkv_epilogue(bias, qn, kn, EPS)
    if path == "qkv":
        q = torch.randn(T, row_w, device="cuda", generator=g).to(dtype)
        x = q + bias
        ops.rope_kv_append_ex(q, pos, cos, sin, kc, vt, 0, H=H, Hkv=Hkv, d=d, epi=epi)
        q = q[:, :H * d]
    else:
        parts = torch.randn(4, T, row_w, device="cuda", generator=g)
        x = (parts[0] + parts[1] + parts[2] + parts[3] + bias.float()).to(dtype)
        q = torch.empty(T, H * d, dtype=dtype, device="cuda")
        ops.rope_kv_append_parts_ex(parts, 4, q, pos, cos, sin, kc, vt, T, 0, H=H, Hkv=Hkv, d=d, epi=epi)
    torch.cuda.synchronize()
    zq = _head_norm(x[:, :H * d].view(T, H, d), qn)
    zk = _head_norm(x[:, H * d:(H + Hkv) * d].view(T, Hkv, d), kn)
    for got, z, what in ((q.view(T, H, d), zq, "q"), (kc[:, :T].transpose(0, 1), zk, "k")):
        diff = (got.float() - z.float()).abs()
        assert bool((diff <= ULPS_Z[dtype] * _ulp(z, dtype) * 1.0001).all()), (what, dtype, H, d, path, diff.max().item())
