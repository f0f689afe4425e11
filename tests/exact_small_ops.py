"""Exact (fp64) models of the small memory-bound ops, the one comparison rule, and the case lists
that tests/test_small_ops_models_cpu.py (ops.* on CPU tensors = ops/reference.py, c = 1) and
tests/test_norm_act_gpu.py / tests/test_moe_dispatch_gpu.py (the HIP kernels, c = 8) both run.

The models are written out in the obvious way in fp64 over the bf16 / fp32 inputs, share no code
with ops/reference.py, return fp64 and never round to bf16.

The rule (docs/development.md): a kernel computes in fp32 and rounds once to bf16, so against the
fp64 value r every output y satisfies

    |y - r| <= halfulp_bf16(r) + c * 2^-24 * A + 2^-126

halfulp_bf16(r) = 2^(e-8) for |r| in [2^e, 2^(e+1)) is the one final rounding; 2^-126 (the smallest
normal) lets a kernel flush a subnormal result; A is the magnitude before any cancellation (given
per op below) and c the number of fp32 roundings of that magnitude the computation may spend:
c = 1 for the fp32 CPU reference, c = 8 for a kernel (another reduction tree, 1-ulp intrinsics).
Outputs that are copies or integers (the fused-add residual, embedding, gather_rows, resolve_ids,
expert ids, every moe_align output) are compared with torch.equal.
"""
import math
import struct
import zlib

import torch

from k8s_llm_monitor_amd import ops

BF16 = torch.bfloat16
C_REF = 1.0  # ops.reference on the CPU
C_GPU = 8.0  # the HIP kernels


# ------------------------------------------------------------------------------ the rule

def halfulp_bf16(r: torch.Tensor) -> torch.Tensor:
    """Half a bf16 ulp at r (fp64): 2^(e-8) for |r| in [2^e, 2^(e+1)), e floored at -126; 0 at 0."""
    r = r.double()
    _, ex = torch.frexp(r)  # |r| = m * 2^ex with m in [0.5, 1): e = ex - 1
    e = (ex - 1).clamp(min=-126)
    h = torch.ldexp(torch.ones_like(r), e - 8)
    return torch.where(r == 0, torch.zeros_like(r), h)


def used_c(y: torch.Tensor, r: torch.Tensor, A: torch.Tensor) -> float:
    """The smallest c with which y passes the rule (0 when the rounding term alone covers y)."""
    y, r, A = y.detach().cpu().double(), r.double(), A.double().expand_as(r)
    over = (y - r).abs() - halfulp_bf16(r) - 2.0 ** -126
    over = torch.where(torch.isnan(over), torch.full_like(over, math.inf), over)
    unit = 2.0 ** -24 * A
    need = torch.where(over > 0, over / unit.clamp(min=1e-300), torch.zeros_like(over))
    return float(need.max()) if need.numel() else 0.0


def assert_rule(y: torch.Tensor, r: torch.Tensor, A: torch.Tensor, c: float, what: str) -> float:
    """Assert the rule for every element; returns the c the output needed (for reporting)."""
    assert y.dtype == BF16 and tuple(y.shape) == tuple(r.shape), f"{what}: dtype/shape {y.dtype} {tuple(y.shape)}"
    yd, rd, Ad = y.detach().cpu().double(), r.double(), A.double().expand_as(r)
    err = (yd - rd).abs()
    tol = halfulp_bf16(rd) + c * 2.0 ** -24 * Ad + 2.0 ** -126
    bad = ~(err <= tol)  # NaN / inf outputs are bad
    need = used_c(y, r, A)
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} outside the rule at c={c:g} (needs c={need:.3g}); first at "
            f"flat {i}: got {yd.reshape(-1)[i].item()!r}, exact {rd.reshape(-1)[i].item()!r}, "
            f"tol {tol.reshape(-1)[i].item():.3g}")
    return need


def fails_rule(y: torch.Tensor, r: torch.Tensor, A: torch.Tensor, c: float) -> int:
    """How many elements of y are outside the rule (for showing that a case discriminates)."""
    yd, rd = y.detach().cpu().double(), r.double()
    tol = halfulp_bf16(rd) + c * 2.0 ** -24 * A.double().expand_as(rd) + 2.0 ** -126
    return int((~((yd - rd).abs() <= tol)).sum())


def f32(v: float) -> float:
    """v as the kernel sees it (the binding narrows eps to fp32)."""
    return struct.unpack("f", struct.pack("f", v))[0]


def gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------ models: norms

def rms_norm_model(x, w, eps):
    xd = x.double()
    inv = 1.0 / torch.sqrt((xd * xd).sum(-1, keepdim=True) / x.shape[-1] + f32(eps))
    return xd * inv * w.double()


def fused_sum_model(x, residual):
    """The new residual: the fp32 sum of the two bf16 streams, rounded to bf16."""
    return (x.float() + residual.float()).to(BF16)


def fused_add_rms_norm_model(x, residual, w, eps, rounded=True):
    """(norm, residual).  rounded=False is the *wrong* model (norm of the unrounded sum), kept to
    show that the fused-add case tells the two apart."""
    s = fused_sum_model(x, residual)
    return rms_norm_model(s if rounded else x.double() + residual.double(), w, eps), s


def layer_norm_model(x, w, b, eps):
    """Two-pass; returns (value, A) with A = (|x| + |mean|) * inv * |w| + |b|."""
    xd = x.double()
    d = x.shape[-1]
    mean = xd.sum(-1, keepdim=True) / d
    var = ((xd - mean) ** 2).sum(-1, keepdim=True) / d
    inv = 1.0 / torch.sqrt(var + f32(eps))
    wd, bd = w.double(), b.double()
    return (xd - mean) * inv * wd + bd, (xd.abs() + mean.abs()) * inv * wd.abs() + bd.abs()


# ------------------------------------------------------------------------------ models: activations

def split_gate_up(x, interleaved):
    F = x.shape[-1] // 2
    if not interleaved:
        return x[..., :F], x[..., F:]
    t = x.reshape(*x.shape[:-1], F // 64, 2, 64)
    return t[..., 0, :].reshape(*x.shape[:-1], F), t[..., 1, :].reshape(*x.shape[:-1], F)


def silu_mul_model(x, interleaved=False):
    """Returns (value, A) with A = (1 + |g|) * |value|."""
    g, u = split_gate_up(x.double(), interleaved)
    r = g / (1.0 + torch.exp(-g)) * u
    return r, (1.0 + g.abs()) * r.abs()


def gelu_tanh_model(x):
    """Returns (value, A) with A = |t|."""
    t = x.double()
    u = math.sqrt(2.0 / math.pi) * (t + 0.044715 * t * t * t)
    return 0.5 * t * (1.0 + torch.tanh(u)), t.abs()


# ------------------------------------------------------------------------------ models: gathers

def embedding_model(ids, weight, vocab_start):
    out = torch.zeros(ids.numel(), weight.shape[1], dtype=weight.dtype)
    for t, i in enumerate(ids.tolist()):
        if vocab_start <= i < vocab_start + weight.shape[0]:
            out[t] = weight[i - vocab_start]
    return out


def resolve_ids_model(ids, src, prev):
    p = prev.tolist()
    return torch.tensor([p[s] if s >= 0 else i for i, s in zip(ids.tolist(), src.tolist())], dtype=torch.int32)


def gather_rows_model(x, idx, div):
    return torch.stack([x[i // div] for i in idx.tolist()])


def moe_combine_model(y, inv_idx, w, T):
    """Returns (value, A) with A = sum_k |w_k * v_k|."""
    K = w.shape[1]
    terms = y.double()[inv_idx.long()].view(T, K, -1) * w.double().unsqueeze(-1)
    return terms.sum(1), terms.abs().sum(1)


# ------------------------------------------------------------------------------ models: routing

def moe_route_model(logits, K, renorm):
    """softmax in fp64; K times the largest untaken logit, the lowest index among equals."""
    x = logits.double()
    T, E = x.shape
    p = torch.exp(x - x.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    taken = torch.zeros(T, E, dtype=torch.bool)
    ids = torch.empty(T, K, dtype=torch.int64)
    rows = torch.arange(T)
    for k in range(K):
        best = torch.full((T,), -1, dtype=torch.int64)
        bv = torch.full((T,), -math.inf, dtype=torch.float64)
        for e in range(E):
            better = ~taken[:, e] & ((best < 0) | (x[:, e] > bv))
            best = torch.where(better, torch.full_like(best, e), best)
            bv = torch.where(better, x[:, e], bv)
        taken[rows, best] = True
        ids[:, k] = best
    w = p.gather(1, ids)
    if renorm:
        w = w / w.sum(-1, keepdim=True)
    return ids.to(torch.int32), w


def moe_router_model(x, router_w, K, renorm):
    """(ids, w, wd, logits): the exact dot product, rounded fp64 -> fp32 -> bf16, then moe_route."""
    lg = (x.double() @ router_w.double().t()).float().to(BF16).double()
    ids, w = moe_route_model(lg, K, renorm)
    wd = torch.zeros(x.shape[0], router_w.shape[0], dtype=torch.float64)
    for t in range(x.shape[0]):
        for k in range(K):
            wd[t, int(ids[t, k])] = w[t, k]
    return ids, w, wd, lg


def moe_align_model(ids, E):
    """Stable sort of the flat pairs by expert: (offsets [E+1], sorted_idx, inv_idx), int32."""
    flat = ids.reshape(-1)
    buckets = [torch.nonzero(flat == e).reshape(-1) for e in range(E)]  # ascending = stable
    offsets = [0]
    for b in buckets:
        offsets.append(offsets[-1] + b.numel())
    sorted_idx = torch.cat(buckets)
    inv = torch.empty_like(sorted_idx)
    inv[sorted_idx] = torch.arange(sorted_idx.numel())
    return torch.tensor(offsets, dtype=torch.int32), sorted_idx.to(torch.int32), inv.to(torch.int32)


def assert_align_invariants(ids, E, offsets, sorted_idx, inv_idx):
    flat, n = ids.reshape(-1).long(), ids.numel()
    offsets, sorted_idx, inv_idx = offsets.cpu().long(), sorted_idx.cpu().long(), inv_idx.cpu().long()
    assert offsets.numel() == E + 1 and int(offsets[0]) == 0 and int(offsets[E]) == n
    assert bool((offsets[1:] >= offsets[:-1]).all()), "offsets not monotone"
    assert torch.equal(sorted_idx.sort().values, torch.arange(n)), "sorted_idx is not a permutation"
    ex = flat[sorted_idx]
    assert bool((ex[1:] >= ex[:-1]).all()), "experts of sorted_idx decrease"
    same = ex[1:] == ex[:-1]
    assert bool((sorted_idx[1:][same] > sorted_idx[:-1][same]).all()), "order within an expert is not stable"
    assert torch.equal(inv_idx[sorted_idx], torch.arange(n)), "inv_idx[sorted_idx[p]] != p"
    for e in range(E):
        assert bool((ex[int(offsets[e]):int(offsets[e + 1])] == e).all()), f"segment of expert {e}"


def logit_spread(logits):
    """Per row: largest minus smallest finite logit."""
    x = logits.double()
    fin = torch.isfinite(x)
    hi = torch.where(fin, x, torch.full_like(x, -math.inf)).max(-1).values
    lo = torch.where(fin, x, torch.full_like(x, math.inf)).min(-1).values
    return hi - lo


def assert_route_weights(w, wm, spread, renorm, what):
    """Routing weights (fp32) against the fp64 model at the project's tolerance (rtol 1e-5, atol
    1e-6; rtol x spread/16 on rows whose logits span more than 16: the exp argument's rounding
    grows with |x|), and finite, >= 0, summing to 1 when renormalised."""
    assert w.dtype == torch.float32, what
    wd = w.detach().cpu().double()
    assert bool(torch.isfinite(wd).all()), f"{what}: non-finite weight"
    assert bool((wd >= 0).all()), f"{what}: negative weight"
    rtol = 1e-5 * (spread / 16.0).clamp(min=1.0).unsqueeze(-1)
    err = (wd - wm).abs()
    bad = ~(err <= 1e-6 + rtol * wm.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())} weights out of tolerance, max err {float(err.max()):.3g}"
    if renorm:
        s = wd.sum(-1)
        assert bool(((s - 1.0).abs() <= 1e-5).all()), f"{what}: renormalised weights sum to {s.min()}..{s.max()}"


# ------------------------------------------------------------------------------ cases: norms

RMS_D = (8, 768, 2048, 2056, 4096, 5120, 6144, 8192, 8200, 16384)
LN_D = (8, 768, 2048, 2056, 4096, 8192)
NORM_ROWS = (1, 3)
NORM_FAMILIES = ("unit", "small_eps5", "small_eps6", "scale100", "outlier", "zero_row")
FUSED_FAMILIES = NORM_FAMILIES + ("resid256",)  # residual ~ 256 randn, x ~ randn: the rounding of the sum shows
LN_FAMILIES = NORM_FAMILIES + ("offset64",)


def norm_input(family, rows, d, g):
    """(x bf16 [rows, d], eps)."""
    x = torch.randn(rows, d, generator=g, dtype=torch.float64)
    eps = 1e-5
    if family in ("small_eps5", "small_eps6"):
        x *= 1e-3
        eps = 1e-5 if family == "small_eps5" else 1e-6
    elif family == "scale100":
        x *= 100.0
    elif family == "outlier":
        for r in range(rows):
            x[r, (r * 977 + 5) % d] = 2.0 ** 14
    elif family == "zero_row":
        x[0] = 0.0
    elif family == "offset64":
        x += 64.0
    return x.to(BF16), eps


def _nan_out(shape, dev):
    return torch.full(shape, float("nan"), dtype=BF16, device=dev)


def check_rms_norm(dev, c, d, family, fused):
    """Every row count of one (d, family); returns the largest c any output needed."""
    worst = 0.0
    for rows in NORM_ROWS:
        g = gen("rms", d, family, rows, fused)
        w = torch.randn(d, generator=g).to(BF16)
        what = f"rms_norm d={d} rows={rows} {family} fused={fused}"
        out = _nan_out((rows, d), dev)
        if fused:
            if family == "resid256":
                x = torch.randn(rows, d, generator=g).to(BF16)
                res = (256.0 * torch.randn(rows, d, generator=g)).to(BF16)
                eps = 1e-5
            else:
                x, eps = norm_input(family, rows, d, g)
                res, _ = norm_input(family, rows, d, g)
            r, s = fused_add_rms_norm_model(x, res, w, eps)
            res_dev = res.clone().to(dev)
            y = ops.fused_add_rms_norm(x.to(dev), res_dev, w.to(dev), eps, out=out)
            assert torch.equal(res_dev.cpu(), s), f"{what}: residual is not bf16(x + residual)"
        else:
            x, eps = norm_input(family, rows, d, g)
            r = rms_norm_model(x, w, eps)
            y = ops.rms_norm(x.to(dev), w.to(dev), eps, out=out)
        worst = max(worst, assert_rule(y, r, r.abs(), c, what))
        if family == "zero_row":
            assert bool((y[0].cpu() == 0).all()), f"{what}: the all-zero row must give exactly 0"
    return worst


def check_rms_norm_strided(dev, c, d, fused):
    """x and out are column slices [:, 8:8+d] of wider matrices; the rest of out stays untouched."""
    rows, wide = 3, d + 24
    g = gen("rms_strided", d, fused)
    xw = torch.randn(rows, wide, generator=g).to(BF16)
    w = torch.randn(d, generator=g).to(BF16)
    x = xw[:, 8:8 + d]
    ow = torch.full((rows, wide), 7.0, dtype=BF16).to(dev)
    out = ow[:, 8:8 + d]
    what = f"strided rms_norm d={d} fused={fused}"
    if fused:
        res = (256.0 * torch.randn(rows, d, generator=g)).to(BF16)
        r, s = fused_add_rms_norm_model(x, res, w, 1e-5)
        res_dev = res.clone().to(dev)
        ops.fused_add_rms_norm(xw.to(dev)[:, 8:8 + d], res_dev, w.to(dev), 1e-5, out=out)
        assert torch.equal(res_dev.cpu(), s), f"{what}: residual"
    else:
        r = rms_norm_model(x, w, 1e-5)
        ops.rms_norm(xw.to(dev)[:, 8:8 + d], w.to(dev), 1e-5, out=out)
    used = assert_rule(out, r, r.abs(), c, what)
    o = ow.cpu()
    assert bool((o[:, :8] == 7.0).all()) and bool((o[:, 8 + d:] == 7.0).all()), f"{what}: wrote outside the slice"
    return used


def check_layer_norm(dev, c, d, family):
    worst = 0.0
    for rows in NORM_ROWS:
        g = gen("ln", d, family, rows)
        x, eps = norm_input(family, rows, d, g)
        w = torch.randn(d, generator=g).to(BF16)
        b = torch.randn(d, generator=g).to(BF16)
        r, A = layer_norm_model(x, w, b, eps)
        y = ops.layer_norm(x.to(dev), w.to(dev), b.to(dev), eps)
        what = f"layer_norm d={d} rows={rows} {family}"
        worst = max(worst, assert_rule(y, r, A, c, what))
        if family == "zero_row":
            assert torch.equal(y[0].cpu(), b), f"{what}: the all-zero row must give exactly the bias"
    return worst


# ------------------------------------------------------------------------------ cases: activations

SILU_F = (8, 64, 2048, 2056, 3584)
SILU_CASES = tuple((F, il) for F in SILU_F for il in (False, True) if not il or F % 64 == 0)
SILU_ROWS = (1, 5)
SILU_LONG = ((65539, 8, False), (65539, 64, True))  # rows > 65535: the kernel's row loop
SILU_GATES = (-1e4, -100.0, -88.5, -87.0, -20.0, -1.0, -0.0, 0.0, 1.0, 20.0, 88.0, 100.0, 1e4)
SILU_UPS = (3.0, -3.0, 1e4)
GELU_N = (8, 307200, 2048 * 256 * 8 + 8 * 300)  # the last one: past the 2048-block grid, grid-stride
GELU_SWEEP = (-1e15, -1e4, -10.0, -6.0, -5.0, -3.0, -0.0, 0.0, 3.0, 10.0, 1e4, 1e15)


def _silu_run(dev, c, x, interleaved, what):
    r, A = silu_mul_model(x, interleaved)
    out = _nan_out(tuple(r.shape), dev)
    y = ops.silu_mul(x.to(dev), out=out, interleaved=interleaved)
    return assert_rule(y, r, A, c, what)


def check_silu_mul(dev, c, F, interleaved):
    worst = 0.0
    for rows in SILU_ROWS:
        x = (2.0 * torch.randn(rows, 2 * F, generator=gen("silu", F, rows, interleaved))).to(BF16)
        worst = max(worst, _silu_run(dev, c, x, interleaved, f"silu_mul F={F} rows={rows} il={interleaved}"))
    return worst


def check_silu_mul_long(dev, c, rows, F, interleaved):
    x = (2.0 * torch.randn(rows, 2 * F, generator=gen("silu_long", F, interleaved))).to(BF16)
    return _silu_run(dev, c, x, interleaved, f"silu_mul F={F} rows={rows} il={interleaved}")


def check_silu_mul_sweep(dev, c, interleaved):
    """Every gate of SILU_GATES against every up of SILU_UPS in one row of F = 64 (zero padded)."""
    pairs = [(gv, uv) for gv in SILU_GATES for uv in SILU_UPS]
    F = 64
    gate, up = torch.zeros(F), torch.zeros(F)
    gate[:len(pairs)] = torch.tensor([p[0] for p in pairs])
    up[:len(pairs)] = torch.tensor([p[1] for p in pairs])
    x = torch.cat([gate, up]).to(BF16).reshape(1, 2 * F)  # [64 gate | 64 up] is both layouts at F = 64
    return _silu_run(dev, c, x, interleaved, f"silu_mul gate sweep il={interleaved}")


def check_gelu(dev, c, n):
    x = (3.0 * torch.randn(n, generator=gen("gelu", n))).to(BF16)
    r, A = gelu_tanh_model(x)
    return assert_rule(ops.gelu_tanh(x.to(dev)), r, A, c, f"gelu_tanh n={n}")


def check_gelu_sweep(dev, c):
    x = torch.tensor(GELU_SWEEP + (0.0,) * (16 - len(GELU_SWEEP))).to(BF16)
    r, A = gelu_tanh_model(x)
    return assert_rule(ops.gelu_tanh(x.to(dev)), r, A, c, "gelu_tanh sweep")


# ------------------------------------------------------------------------------ cases: gathers

EMB_D = (8, 512, 2048, 2056, 4096)
RESOLVE_N = (65, 200)
GATHER_D = (8, 2048, 2056, 4096, 6144)
GATHER_DIV = (1, 2, 4)
COMBINE_K = (1, 2, 4, 8)


def check_embedding(dev, d):
    g = gen("emb", d)
    V, start = 37, 100
    weight = torch.randn(V, d, generator=g).to(BF16)
    ids = torch.cat([torch.tensor([99, 100, 136, 137, -1, 0, 50, 5000, 118]),
                     torch.randint(start, start + V, (8,), generator=g)]).to(torch.int32)
    y = ops.embedding(ids.to(dev), weight.to(dev), vocab_start=start)
    assert torch.equal(y.cpu(), embedding_model(ids, weight, start)), f"embedding d={d}"


def check_resolve_ids(dev, n):
    g = gen("resolve", n)
    ids = torch.randint(0, 50000, (n,), generator=g).to(torch.int32)
    prev = torch.randint(0, 50000, (n + 3,), generator=g).to(torch.int32)
    src = torch.randint(-1, n + 3, (n,), generator=g).to(torch.int32)
    src[::3] = -1
    y = ops.resolve_ids(ids.to(dev), src.to(dev), prev.to(dev))
    assert torch.equal(y.cpu(), resolve_ids_model(ids, src, prev)), f"resolve_ids n={n}"


def check_gather_rows(dev, d, div):
    g = gen("gather", d, div)
    R, n = 9, 23
    x = torch.randn(R, d, generator=g).to(BF16)
    idx = torch.randint(0, R * div, (n,), generator=g).to(torch.int32)
    idx[0], idx[1] = 0, R * div - 1
    y = ops.gather_rows(x.to(dev), idx.to(dev), div)
    assert torch.equal(y.cpu(), gather_rows_model(x, idx, div)), f"gather_rows d={d} div={div}"


def check_moe_combine(dev, c, d, K, renorm):
    g = gen("combine", d, K, renorm)
    T = 5
    y = torch.randn(T * K, d, generator=g).to(BF16)
    inv = torch.randperm(T * K, generator=g).to(torch.int32)
    w = torch.rand(T, K, generator=g) + 0.05
    w = (w / w.sum(-1, keepdim=True) if renorm else w * 0.3).float()
    r, A = moe_combine_model(y, inv, w, T)
    out = ops.moe_combine(y.to(dev), inv.to(dev), w.to(dev), T)
    return assert_rule(out, r, A, c, f"moe_combine d={d} K={K} renorm={renorm}")


# ------------------------------------------------------------------------------ cases: routing

ROUTE_EK = ((1, 1), (2, 1), (8, 2), (8, 8), (16, 4), (17, 2), (60, 4), (64, 8), (64, 64))
ROUTE_T = (1, 255, 256, 257)
ROUTE_FAMILIES = ("randn", "ints", "spread80", "neginf")
ROUTE_UNTIED = ("randn",)  # no two logits of a row are equal: the CPU comparison leaves no row out
ROUTER_D = (8, 2048, 2056, 4096, 6144)
ROUTER_E = (1, 2, 7, 8, 9, 16)
ROUTER_T = (1, 5)


def route_logits(family, T, E, g):
    if family == "randn":
        x = 2.0 * torch.randn(T, E, generator=g)
    elif family == "ints":
        x = torch.randint(-2, 3, (T, E), generator=g).float()
    elif family == "spread80":
        x = 160.0 * torch.rand(T, E, generator=g) - 80.0
    else:  # some experts at -inf, at least one finite per row
        x = 2.0 * torch.randn(T, E, generator=g)
        drop = torch.rand(T, E, generator=g) < 0.4
        drop[torch.arange(T), torch.arange(T) % E] = False
        x[drop] = -math.inf
    return x.float()


def ref_tied_rows(logits, K):
    """Rows where the fp32 softmax torch.topk selects from has equal values among its K + 1
    largest (equal logits, or probabilities that underflow to 0): torch.topk promises no order
    there, so ref.moe_route may legitimately name other experts than the lowest-index rule."""
    p = torch.softmax(logits.float(), -1).sort(-1, descending=True).values
    j = min(K + 1, p.shape[1])
    return (p[:, 1:j] == p[:, :j - 1]).any(-1) if j > 1 else torch.zeros(p.shape[0], dtype=torch.bool)


def _assert_route(ids, w, mids, mw, logits, K, renorm, exact_ids, what):
    """ids / w from ops against the model's; exact_ids: bool per row, compare ids there."""
    ids = ids.cpu()
    assert ids.dtype == torch.int32 and tuple(ids.shape) == tuple(mids.shape), what
    E = logits.shape[1]
    assert bool(((ids >= 0) & (ids < E)).all()), f"{what}: id out of range"
    assert all(len(set(r)) == K for r in ids.tolist()), f"{what}: repeated expert in a row"
    assert torch.equal(ids[exact_ids], mids[exact_ids]), f"{what}: expert ids differ from the lowest-index-first model"
    assert_route_weights(w, mw, logit_spread(logits), renorm, what)
    # an expert at -inf weighs exactly 0 and is chosen only once every finite one is
    chosen = logits.gather(1, ids.long())
    dead = chosen == -math.inf
    assert bool((w.cpu()[dead] == 0).all()), f"{what}: an expert at -inf has weight"
    n_fin = torch.isfinite(logits).sum(-1)
    assert torch.equal(dead.sum(-1), (K - n_fin).clamp(min=0)), f"{what}: -inf chosen before a finite expert"


def check_moe_route(dev, E, K, family):
    """Every T and both renorm settings; returns the number of rows whose ids were not compared."""
    left_out = 0
    for T in ROUTE_T:
        lg = route_logits(family, T, E, gen("route", family, T, E, K))
        if family in ROUTE_UNTIED:
            s = lg.sort(-1).values
            assert not bool((s[:, 1:] == s[:, :-1]).any()), "the untied generator produced a tie"
        exact = torch.ones(T, dtype=torch.bool) if dev != "cpu" else ~ref_tied_rows(lg, K)
        left_out += int((~exact).sum())
        for renorm in (True, False):
            mids, mw = moe_route_model(lg, K, renorm)
            ids, w = ops.moe_route(lg.to(dev), K, renorm)
            _assert_route(ids, w, mids, mw, lg, K, renorm, exact, f"moe_route E={E} K={K} T={T} {family} renorm={renorm}")
    return left_out


def router_inputs(T, d, E, g):
    """Small integers (x 2^-7 for the router): every partial sum is exact in fp32 whatever the
    order, so the bf16 logit is determined."""
    x = torch.randint(-2, 3, (T, d), generator=g).to(BF16)
    wr = (torch.randint(-8, 9, (E, d), generator=g).float() / 128).to(BF16)
    return x, wr


def check_moe_router(dev, d, E):
    left_out = 0
    for T in ROUTER_T:
        x, wr = router_inputs(T, d, E, gen("router", T, d, E))
        for K in sorted({1, min(2, E), E}):
            for renorm in (True, False):
                mids, mw, mwd, lg = moe_router_model(x, wr, K, renorm)
                exact = torch.ones(T, dtype=torch.bool) if dev != "cpu" else ~ref_tied_rows(lg, K)
                left_out += int((~exact).sum())
                ids, w, wd = ops.moe_router(x.to(dev), wr.to(dev), K, renorm)
                what = f"moe_router d={d} E={E} K={K} T={T} renorm={renorm}"
                _assert_route(ids, w, mids, mw, lg.float(), K, renorm, exact, what)
                # the dense rows: the same weights at the chosen experts, exact zeros elsewhere
                wd, ids = wd.cpu(), ids.cpu()
                assert wd.dtype == torch.float32 and tuple(wd.shape) == (T, E), what
                assert torch.equal(wd.gather(1, ids.long()), w.cpu()), f"{what}: wd at the chosen experts != w"
                rest = torch.ones(T, E, dtype=torch.bool).scatter_(1, ids.long(), False)
                assert bool((wd[rest] == 0).all()), f"{what}: wd not zero at an unchosen expert"
                sp = logit_spread(lg)
                rtol = 1e-5 * (sp / 16.0).clamp(min=1.0).unsqueeze(-1)
                ok = (wd.double() - mwd).abs() <= 1e-6 + rtol * mwd.abs()
                assert bool(ok[exact].all()), f"{what}: dense weights differ from the model"
    return left_out


ALIGN_N = (1, 1023, 1024, 1025, 2053, 32768, 131072)
ALIGN_E = (1, 3, 8, 16)
ALIGN_FAMILIES = ("uniform", "all_first", "all_last", "ends_empty")


def align_ids(family, n, E, g):
    if family == "uniform":
        ids = torch.randint(0, E, (n,), generator=g)
    elif family == "all_first":
        ids = torch.zeros(n, dtype=torch.int64)
    elif family == "all_last":
        ids = torch.full((n,), E - 1, dtype=torch.int64)
    elif family == "ends_empty":  # nobody routes to the first or the last expert
        ids = torch.randint(1, E - 1, (n,), generator=g) if E >= 3 else torch.zeros(n, dtype=torch.int64)
    else:  # "one_each": one pair per expert, in a shuffled order
        ids = torch.randperm(E, generator=g)
    assert int(ids.min()) >= 0 and int(ids.max()) < E
    return ids.to(torch.int32)


def _align_run(dev, ids, E, what):
    off, srt, inv = ops.moe_align(ids.to(dev), E)
    for t in (off, srt, inv):
        assert t.dtype == torch.int32, what
    assert_align_invariants(ids, E, off, srt, inv)
    moff, msrt, minv = moe_align_model(ids, E)
    assert torch.equal(off.cpu(), moff), f"{what}: offsets"
    assert torch.equal(srt.cpu(), msrt), f"{what}: sorted_idx"
    assert torch.equal(inv.cpu(), minv), f"{what}: inv_idx"


def check_moe_align(dev, n, E):
    for family in ALIGN_FAMILIES:
        _align_run(dev, align_ids(family, n, E, gen("align", family, n, E)), E, f"moe_align n={n} E={E} {family}")


def check_moe_align_one_each(dev, E):
    _align_run(dev, align_ids("one_each", E, E, gen("align1", E)), E, f"moe_align one pair per expert E={E}")


def check_moe_chain(dev, c, T, K, E=8, d=2056):
    """route -> align -> gather -> (identity expert) -> combine with renormalised weights returns
    every input row: the weights of a row sum to 1, so A = sum_k |w_k x| = |x|."""
    g = gen("chain", T, K)
    x = torch.randn(T, d, generator=g).to(BF16)
    lg = 2.0 * torch.randn(T, E, generator=g)
    xd = x.to(dev)
    ids, w = ops.moe_route(lg.to(dev), K, True)
    mids, _ = moe_route_model(lg, K, True)
    assert torch.equal(ids.cpu(), mids)  # in range before they index anything
    off, srt, inv = ops.moe_align(ids, E)
    assert_align_invariants(ids.cpu(), E, off, srt, inv)
    rows = ops.gather_rows(xd, srt, K)
    assert torch.equal(rows.cpu(), x[srt.cpu().long() // K]), "gather_rows in expert order"
    out = ops.moe_combine(rows, inv, w, T)
    return assert_rule(out, x.double(), x.double().abs(), c, f"route-align-gather-combine T={T} K={K}")
