"""lora_shrink_kernel / lora_expand_kernel (ops/csrc/lora.hip) through ops.lora_slab and ops.lora_add
against ops/reference.py lora_delta in fp64.

Shapes: K in {512, 1536} (one and three ss_part columns; 1536 is no power of two), N in {512, 1536},
M in {1, 15, 16, 17, 64, 128} (below, at and above one 16-row tile; one and two expand row groups; the
whole 8 m-tiles of a shrink workgroup).  The arena holds three adapters of ranks 1, 8 and 64 in a
capacity of 64; a second arena holds the fused qkv form at capacity 192 (q, k, v at rank offsets 0, 64,
128 with B block-diagonal over their output ranges).  Slot patterns: all -1, all the same adapter, and
(-1, 0, 1, 2) cycling so that every 16-row tile mixes adapters.  Every case runs the slab form from
the fragment-packed operand and from row-major rows, each with and without the deferred norm, and the
in-place bf16 add from row-major rows.

Bounds (derived, not tuned).  Slab: |err| <= (K + R + 8) 2^-24 (|s| |B| |A| |x|), the last factor taken
element-wise with absolute values: both sums run in fp32 over bf16 inputs and t is never rounded to
bf16.  Add: |out - (y + delta_ref)| <= 2^-8 |y + delta_ref| (one bf16 rounding) plus that bound.

Also: rows without an adapter are exact zeros (slab) or bit-unchanged (add); guard words before and
after every output are unchanged; two launches are bit-identical; the plan's S is the partial count
the kernel wrote."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLACK = 1024
RANKS = (1, 8, 64)
SCALING = (2.0, 0.5, 0.25)
EPS = 1e-5
U24 = 2.0 ** -24


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    for c in (_state, _x, _ss):
        c.cache_clear()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _state(N, K, qkv=False):
    """One layer, three adapters.  Plain: ranks 1, 8, 64 in capacity 64.  qkv: capacity 192, every
    adapter q / k / v blocks of its rank at rank offsets 0, 64, 128 over N/2, N/4, N/4 output rows."""
    st = ops.LoraState(3, 1, {"wqkv" if qkv else "wo": (N, K, 192 if qkv else 64)}, DEV)
    g = _gen(N * 31 + K + (5 if qkv else 0))
    for s, r in enumerate(RANKS):
        st.set_scaling(s, SCALING[s])
        parts = ((0, N // 2), (N // 2, N // 4), (3 * N // 4, N // 4)) if qkv else ((0, N),)
        for j, (n0, n) in enumerate(parts):
            A = (torch.randn(r, K, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
            B = (torch.randn(n, r, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
            st.load(s, 0, "wqkv" if qkv else "wo", A, B, r0=64 * j, n0=n0)
    return st


@functools.lru_cache(maxsize=None)
def _x(M, K):
    return torch.randn(M, K, device=DEV, generator=_gen(M * 7919 + K)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _ss(M, K):
    return (torch.rand(M, K // 512, device=DEV, generator=_gen(M + K)) + 0.25) * (K / 2)


def _slots(pattern, M):
    if pattern == "none":
        v = [-1] * M
    elif pattern.startswith("same"):
        v = [int(pattern[4:])] * M
    else:
        v = [(-1, 0, 1, 2)[(i + 1) % 4] for i in range(M)]  # row 0 has an adapter
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _sentinel(n):
    return (torch.arange(n, device=DEV, dtype=torch.float32) % 251.0) - 125.5


def _reference(st, proj, M, K, slot, norm):
    """(delta in fp64, the bound's |s| |B| |A| |x|) with the deferred norm folded into x."""
    x = _x(M, K).double()
    if norm:
        x = x * torch.rsqrt(_ss(M, K).double().sum(1, keepdim=True) / K + EPS)
    A, B = st.A[proj][0], st.B[proj][0]
    d = ref.lora_delta(x, A, B, st.scaling, slot, dtype=torch.float64)
    mag = ref.lora_delta(x.abs(), A.abs(), B.abs(), st.scaling.abs(), slot, dtype=torch.float64)
    return d, mag


def _check(M, N, K, pattern, qkv):
    st = _state(N, K, qkv)
    proj = "wqkv" if qkv else "wo"
    R = st.dims[proj][2]
    slot = _slots(pattern, M)
    off = slot < 0
    x = _x(M, K)
    ns = 2
    first = None
    for norm in (False, True):
        d, mag = _reference(st, proj, M, K, slot, norm)
        bound = (K + R + 8) * U24 * mag
        rn = (_ss(M, K), EPS) if norm else None
        for packed in (True, False):
            ws = _sentinel((ns + 1) * M * N + SLACK)
            want = ws.clone()
            a = ops.pack_activation(x) if packed else x
            assert ops.lora_slab(st, 0, proj, a, M, ws, ns, slot, rownorm=rn) == ns + 1
            got = ws[ns * M * N:(ns + 1) * M * N].view(M, N)
            assert torch.equal(ws[:ns * M * N], want[:ns * M * N]), "slabs before the new one changed"
            assert torch.equal(ws[(ns + 1) * M * N:], want[(ns + 1) * M * N:]), "words after the slab changed"
            assert torch.equal(got[off], torch.zeros_like(got[off])), "rows without an adapter must be zeros"
            err = (got.double() - d).abs()
            print(f"slab M={M} N={N} K={K} {pattern} norm={norm} packed={packed}: max err {err.max().item():.3e} "
                  f"max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
            assert bool((err <= bound).all())
            ws2 = _sentinel((ns + 1) * M * N + SLACK)
            ops.lora_slab(st, 0, proj, a, M, ws2, ns, slot, rownorm=rn)
            assert torch.equal(ws, ws2), "two launches differ"
            if not norm:
                if first is None:
                    first = got.clone()
                else:  # the two input forms feed the same fragments: the same bits
                    assert torch.equal(first, got)
    # in-place bf16 add from row-major rows, guard rows around y
    d, mag = _reference(st, proj, M, K, slot, False)
    buf = (torch.randn(M + 2, N, device=DEV, generator=_gen(M + N)) * 0.5).to(torch.bfloat16)
    before = buf.clone()
    y = buf[1:M + 1]
    ops.lora_add(st, 0, proj, x, y, slot)
    assert torch.equal(buf[0], before[0]) and torch.equal(buf[M + 1], before[M + 1]), "guard rows changed"
    assert torch.equal(y[off], before[1:M + 1][off]), "rows without an adapter must be untouched"
    target = before[1:M + 1].double() + d
    err = (y.double() - target).abs()
    lim = 2.0 ** -8 * target.abs() + (K + R + 8) * U24 * mag
    print(f"add  M={M} N={N} K={K} {pattern}: max err {err[~off].max().item() if bool((~off).any()) else 0.0:.3e}")
    assert bool((err[~off] <= lim[~off]).all())
    buf2 = before.clone()
    ops.lora_add(st, 0, proj, x, buf2[1:M + 1], slot)
    assert torch.equal(buf, buf2), "two launches differ"


@pytest.mark.parametrize("pattern", ["none", "same2", "cycle"])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 64, 128])
@pytest.mark.parametrize("N,K", [(512, 512), (1536, 512), (512, 1536), (1536, 1536)])
def test_lora_kernels(N, K, M, pattern):
    _check(M, N, K, pattern, qkv=False)


@pytest.mark.parametrize("same", [0, 1])
def test_lora_small_ranks_alone(same):
    """Every row on the rank-1 (rank-8) adapter: the zero-padded ranks of the capacity."""
    _check(17, 512, 512, f"same{same}", qkv=False)


@pytest.mark.parametrize("pattern", ["none", "same1", "cycle"])
@pytest.mark.parametrize("M", [17, 128])
def test_lora_fused_qkv(M, pattern):
    _check(M, 1536, 512, pattern, qkv=True)


@pytest.mark.parametrize("K", [512, 1536, 4096, 14336])
def test_shrink_plan_is_what_the_kernel_wrote(K):
    """ops.lora_shrink_plan mirrors the binding's plan, and a launch writes exactly that many
    partials: every word of t_part [S, M, R] and none of the slab after it."""
    M, R = 17, 64
    S = ops.lora_shrink_plan(K)
    assert S == ops.native().lora_shrink_plan(K)
    assert 1 <= S <= 16 and (S == 1) == (K < 1024)
    A = (torch.randn(2, R, K, device=DEV, generator=_gen(K)) * 0.05).to(torch.bfloat16)
    slot = _slots("cycle", M)
    mark = 7.0e30  # no product of these inputs
    t = torch.full(((S + 1) * M * R + SLACK,), mark, device=DEV)
    assert ops.native().lora_shrink(_x(M, K), A, slot, t, M, None, 0.0) == S
    assert bool((t[:S * M * R] != mark).all()), "a partial the plan promises was not written"
    assert bool((t[S * M * R:] == mark).all()), "the kernel wrote past S partials"
    # the partials summed in fp64 are A x (slots 0 and 1 exist in this arena; slot 2 is outside it:
    # an out-of-range slot is no adapter)
    tt = t[:S * M * R].view(S, M, R).double().sum(0)
    for i, s in enumerate(slot.tolist()):
        want = A[s].double() @ _x(M, K)[i].double() if 0 <= s < 2 else torch.zeros(R, device=DEV, dtype=torch.float64)
        mag = A[s].double().abs() @ _x(M, K)[i].double().abs() if 0 <= s < 2 else torch.zeros_like(want)
        assert bool(((tt[i] - want).abs() <= (K + 8) * U24 * mag).all())
