"""The fp8 (e4m3) KV cache's kernels: the quantising cache write, paged decode (unfused and fused)
and the v1 paged prefill's fp8 branch.  Head dim 128, 16-token blocks, random block tables.

Every scale is a power of two and an e4m3 value is a bf16 value, so the fp8 read paths must be
BIT-identical to the bf16 kernels run over a cache that holds the dequantised values."""
import math

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
D, BS, HKV = 128, 16, 8
SCALE = 1.0 / math.sqrt(D)
SENT_CODE, SENT_SCALE = 0x5A, 7.0  # 0x5A is a finite e4m3 value


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()


def _close(a, b, what, atol=2e-2, rtol=2e-2):
    a, b = a.float(), b.float()
    bad = (a - b).abs() > atol + rtol * b.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} off, max abs diff {float((a - b).abs().max()):.4g}"


def _sentinel_cache(nb, device=DEV, hkv=HKV):
    k, v, sc = (t[0] for t in ops.kv_cache_alloc(1, nb, hkv, D, F8, device))
    k.view(torch.uint8).fill_(SENT_CODE)
    v.view(torch.uint8).fill_(SENT_CODE)
    sc.fill_(SENT_SCALE)
    return k, v, sc


def _same_cache(got, want, what):
    """Scales equal everywhere (sentinels included) and codes equal as numbers (-0 == +0): with
    equal scales that is equality of the dequantised values.  ``want`` is built on the CPU."""
    for g, w, n in zip(got, want, ("k codes", "v codes", "scales")):
        g, w = g.cpu(), w.cpu()
        assert torch.equal(g.float(), w.float()), f"{what}: {n} differ at {int((g.float() != w.float()).sum())} places"


def _slots(bt_row, start, n):
    pos = torch.arange(start, start + n, device=bt_row.device)
    return (bt_row[pos // BS].long() * BS + pos % BS).to(torch.int32)


@pytest.fixture(scope="module")
def filled():
    """A cache of 640 random blocks, as fp8 and as the bf16 cache of its dequantised values (both
    left unchanged by the tests: writers work on clones)."""
    nb = 640
    g = torch.Generator(device="cpu").manual_seed(11)
    k = torch.randn(nb * BS, HKV, D, generator=g).to(torch.bfloat16)
    v = torch.randn(nb * BS, HKV, D, generator=g).to(torch.bfloat16)
    v[::7] *= 0.02  # token scales that differ inside one block (magnitudes stay those of the bf16
    k[::5] *= 0.05  # tests, whose 2e-2 tolerance the fused cases keep)
    all_slots = torch.arange(nb * BS, dtype=torch.int32)
    k8, v8, sc = (t[0] for t in ops.kv_cache_alloc(1, nb, HKV, D, F8, "cpu"))
    ref.write_kv_cache(k, v, k8, v8, all_slots, sc)  # the CPU reference quantiser
    kd, vd = (t[0] for t in ops.kv_cache_alloc(1, nb, HKV, D, torch.bfloat16, "cpu"))
    ref.write_kv_cache(ops.dequantize_kv(*ops.quantize_kv(k)), ops.dequantize_kv(*ops.quantize_kv(v)), kd, vd, all_slots)
    return {"nb": nb, "f8": (k8.to(DEV), v8.to(DEV), sc.to(DEV)), "bf16": (kd.to(DEV), vd.to(DEV))}


def _tables(B, max_blocks, nb, seed):
    """Distinct random blocks per entry; a read-only case too large for that shares blocks."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if B * max_blocks <= nb:
        t = torch.randperm(nb, generator=g)[: B * max_blocks]
    else:
        t = torch.randint(0, nb, (B * max_blocks,), generator=g)
    return t.view(B, max_blocks).to(torch.int32).to(DEV)


# ------------------------------------------------------------------ the write kernel
def test_cache_write_quantises_runs_and_touches_nothing_else():
    """70 rows: a 37-token run from block offset 5, a 30-token run from offset 0 and three rows
    with slot -1, into a cache of sentinels.  Codes and scales == ops.quantize_kv of the rotated
    bf16 rows; every other byte and scale keeps its sentinel (ragged run ends take byte stores)."""
    hq, nb = 32, 12
    g = torch.Generator(device="cpu").manual_seed(5)
    bt = _tables(2, 4, nb, 5)
    neg = torch.tensor([-1], dtype=torch.int32, device=DEV)
    slots = torch.cat([_slots(bt[0], 5, 37), neg, _slots(bt[1], 0, 30), neg, neg])
    pos = torch.cat([torch.arange(5, 42), torch.tensor([9]), torch.arange(0, 30), torch.tensor([3, 4])]).to(torch.int32).to(DEV)
    T = 70
    assert slots.numel() == T == pos.numel()
    qkv = torch.randn(T, (hq + 2 * HKV) * D, generator=g).to(DEV).to(torch.bfloat16)
    qkv[3] *= 30.0
    qkv[50] *= 1e-3
    cs = ref.rope_cos_sin(4096, D, 500000.0, None, device=DEV)
    got = _sentinel_cache(nb)
    want = _sentinel_cache(nb, "cpu")
    ops.rope_and_cache(qkv, pos, cs, got[0], got[1], slots, hq, HKV, D, kv_scale=got[2])
    torch.cuda.synchronize()
    k = qkv[:, hq * D:(hq + HKV) * D].reshape(T, HKV, D).cpu()  # rotated in place
    v = qkv[:, (hq + HKV) * D:].reshape(T, HKV, D).cpu()
    ref.write_kv_cache(k, v, want[0], want[1], slots.cpu(), want[2])
    _same_cache(got, want, "prefill runs")
    n_sent = int((got[2] == SENT_SCALE).sum())
    assert n_sent == got[2].numel() - 67 * HKV * 2, "exactly the 67 written tokens' scales moved"


def test_cache_write_from_slabs_matches_the_rows_it_leaves():
    """partial= form, 4 single-token rows: the slabs are reduced and rotated into the bf16 rows (v
    included) and the cache holds quantize_kv of exactly those rows."""
    hq, nb, T, S = 32, 6, 4, 3
    g = torch.Generator(device="cpu").manual_seed(6)
    ncol = (hq + 2 * HKV) * D
    part = (torch.randn(S, T, ncol, generator=g) * 0.3).to(DEV)
    pos = torch.tensor([0, 17, 300, 31], dtype=torch.int32, device=DEV)
    slots = torch.tensor([5 * BS + 0, 2 * BS + 1, 0 * BS + 12, 2 * BS + 15], dtype=torch.int32, device=DEV)
    cs = ref.rope_cos_sin(4096, D, 500000.0, None, device=DEV)
    got, want = _sentinel_cache(nb), _sentinel_cache(nb, "cpu")
    qkv = torch.zeros(T, ncol, device=DEV, dtype=torch.bfloat16)
    ops.rope_and_cache(qkv, pos, cs, got[0], got[1], slots, hq, HKV, D, partial=part.reshape(-1), nslabs=S,
                       kv_scale=got[2])
    torch.cuda.synchronize()
    plain = part.sum(0).to(torch.bfloat16)
    ops.rope_and_cache(plain, pos, cs, None, None, None, hq, HKV, D)
    _close(qkv, plain, "reduced + rotated rows", atol=2e-2, rtol=1e-2)
    k = qkv[:, hq * D:(hq + HKV) * D].reshape(T, HKV, D).cpu()
    v = qkv[:, (hq + HKV) * D:].reshape(T, HKV, D).cpu()
    ref.write_kv_cache(k, v, want[0], want[1], slots.cpu(), want[2])
    _same_cache(got, want, "slab form")


# ------------------------------------------------------------------ unfused decode
CYCLE = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300, 700]
DECODE_CASES = {
    "tw64": ([1, 15, 16, 17, 129], 1),               # S Hkv B = 40: the single-buffered 64-token form
    "tw32": ([CYCLE[i % 12] for i in range(48)], 1),  # S Hkv B = 384: the double-buffered 32-token form
    "split": ([2304, 700, 5, 0], 4),                  # the reduce launch and a padding row
}


@pytest.mark.parametrize("case,hq,packed", [("tw64", 32, False), ("tw64", 64, False), ("tw64", 8, False),
                                            ("tw32", 32, False), ("tw32", 8, True), ("split", 32, False),
                                            ("split", 64, False), ("split", 8, False)])
def test_decode_is_bit_identical_to_bf16_over_the_dequantised_cache(filled, case, hq, packed):
    lens, splits = DECODE_CASES[case]
    B = len(lens)
    max_blocks = (max(lens) + BS - 1) // BS
    bt = _tables(B, max_blocks, filled["nb"], 20 + B)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(3)
    q = torch.randn(B, hq * D, generator=g).to(DEV).to(torch.bfloat16)
    k8, v8, sc = filled["f8"]
    kd, vd = filled["bf16"]
    outs = [ops.packed_empty(B, hq * D, torch.bfloat16, DEV) if packed else None for _ in range(2)]
    if packed:
        for o in outs:
            o.zero_()
    y = ops.paged_decode(q, k8, v8, bt, lens_t, hq, HKV, D, SCALE, splits=splits, out=outs[0], kv_scale=sc)
    r = ops.paged_decode(q, kd, vd, bt, lens_t, hq, HKV, D, SCALE, splits=splits, out=outs[1])
    torch.cuda.synchronize()
    assert not torch.isnan(y.float()).any()
    assert torch.equal(y, r), f"{int((y != r).sum())} of {y.numel()} outputs differ"
    if not packed and case != "tw32":
        rr = ref.paged_decode(q.cpu(), k8.cpu(), v8.cpu(), bt.cpu(), lens_t.cpu(), hq, HKV, D, SCALE, kv_scale=sc.cpu())
        # P enters the PV product rounded to bf16 (2^-9 relative) and the output is rounded to bf16
        # again: |error| <= 2^-8 max|v|; twice that for the exp2 and accumulation order
        _close(y.cpu(), rr, "fp8 decode vs fp32 reference", atol=2.0 ** -7 * float(vd.abs().max()), rtol=0.0)


def test_bindings_refuse_an_fp8_cache_without_scales_or_with_head_dim_64(filled):
    k8, v8, sc = filled["f8"]
    bt = _tables(1, 1, 8, 1)
    lens_t = torch.tensor([5], dtype=torch.int32, device=DEV)
    q = torch.zeros(1, 8 * D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="kv_scale"):
        ops.paged_decode(q, k8, v8, bt, lens_t, 8, HKV, D, SCALE, splits=1)
    k64, v64, s64 = (t[0] for t in ops.kv_cache_alloc(1, 8, HKV, 64, F8, DEV))
    with pytest.raises(RuntimeError, match="head_dim 128"):
        ops.paged_decode(q[:, : 8 * 64], k64, v64, bt, lens_t, 8, HKV, 64, 0.125, splits=1, kv_scale=s64)


# ------------------------------------------------------------------ fused decode
def _fused_inputs(lens, hq, nslabs, seed, nb):
    B = len(lens)
    max_blocks = (max(lens) + BS - 1) // BS + 1
    bt = _tables(B, max_blocks, nb, seed)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    pos = (lens_t - 1).clamp(min=0)
    slots = torch.stack([bt[b, max(lens[b] - 1, 0) // BS] * BS + max(lens[b] - 1, 0) % BS for b in range(B)]).to(torch.int32)
    g = torch.Generator(device="cpu").manual_seed(seed)
    slabs = (torch.randn(nslabs, B, (hq + 2 * HKV) * D, generator=g) * 0.5).to(DEV)
    slabs[:, :, (hq + HKV) * D:] *= torch.logspace(-2, 0, B, device=DEV)[None, :, None]  # v scales over 2^-7 .. 1
    return bt, lens_t, pos, slots, slabs


def _rows_at(kc, vc, slots):
    blk, off = slots.long() // BS, slots.long() % BS
    k = kc[blk, :, :, off, :].reshape(slots.numel(), HKV, D)
    v = vc[blk, :, :, ref.v_perm(off)]
    return k, v


@pytest.mark.parametrize("lens,hq,splits", [([1, 2, 17, 256, 257, 700], 32, None), ([300, 77, 1024, 513], 32, 4),
                                            ([40, 600], 64, 1), ([129, 64], 8, 1)])
def test_fused_decode_quantises_the_new_token_and_matches_the_unfused_path(filled, lens, hq, splits):
    """The fused kernel's cache write == quantize_kv of the row the bf16 fused kernel writes for the
    same slabs, exactly (both instantiations round and rotate the slab sum in the same code); its
    output matches rope_and_cache + paged_decode over the fp8 cache and the fp32 reference within
    the tolerance of test_paged_decode_fused_matches_rope_then_decode."""
    nslabs = 2
    bt, lens_t, pos, slots, slabs = _fused_inputs(lens, hq, nslabs, 30 + len(lens), filled["nb"])
    cs = ref.rope_cos_sin(4096, D, 500000.0, None, device=DEV)
    f8 = tuple(t.clone() for t in filled["f8"])
    f8_unfused = tuple(t.clone() for t in filled["f8"])
    bf = tuple(t.clone() for t in filled["bf16"])
    y = ops.paged_decode_fused(slabs.reshape(-1), nslabs, pos, cs, slots, f8[0], f8[1], bt, lens_t, hq, HKV, D, SCALE,
                               splits=splits, kv_scale=f8[2])
    ops.paged_decode_fused(slabs.reshape(-1), nslabs, pos, cs, slots, bf[0], bf[1], bt, lens_t, hq, HKV, D, SCALE,
                           splits=splits)
    torch.cuda.synchronize()
    k_row, v_row = _rows_at(bf[0], bf[1], slots)  # what the bf16 kernel wrote
    want = tuple(t.cpu() for t in filled["f8"])
    ref.write_kv_cache(k_row.cpu(), v_row.cpu(), want[0], want[1], slots.cpu(), want[2])
    _same_cache(f8, want, "fused write")
    # unfused fp8: slabs -> rows + quantised cache write, then paged_decode
    qkv = torch.empty(len(lens), (hq + 2 * HKV) * D, device=DEV, dtype=torch.bfloat16)
    ops.rope_and_cache(qkv, pos, cs, f8_unfused[0], f8_unfused[1], slots, hq, HKV, D, partial=slabs.reshape(-1),
                       nslabs=nslabs, kv_scale=f8_unfused[2])
    r = ops.paged_decode(qkv, f8_unfused[0], f8_unfused[1], bt, lens_t, hq, HKV, D, SCALE, splits=splits,
                         kv_scale=f8_unfused[2])
    _same_cache(f8_unfused, want, "unfused write of the same token")
    _close(y, r, "fused vs rope_and_cache + paged_decode (fp8)")
    rr = ref.paged_decode(qkv.cpu(), f8[0].cpu(), f8[1].cpu(), bt.cpu(), lens_t.cpu(), hq, HKV, D, SCALE,
                          kv_scale=f8[2].cpu())
    _close(y.cpu(), rr, "fused vs fp32 reference over the fp8 cache")


def test_fused_decode_folds_the_quantised_token():
    """lens = [1]: the only token has softmax weight 1, so the output is the new V as folded - it
    must equal the DEQUANTISED v bit for bit (and differ from the unquantised v)."""
    hq, nslabs, nb = 32, 2, 4
    bt, lens_t, pos, slots, slabs = _fused_inputs([1], hq, nslabs, 41, nb)
    cs = ref.rope_cos_sin(4096, D, 500000.0, None, device=DEV)
    f8 = _sentinel_cache(nb)
    y = ops.paged_decode_fused(slabs.reshape(-1), nslabs, pos, cs, slots, f8[0], f8[1], bt, lens_t, hq, HKV, D, SCALE,
                               splits=1, kv_scale=f8[2])
    torch.cuda.synchronize()
    v_plain = slabs[:, 0, (hq + HKV) * D:].sum(0).to(torch.bfloat16).view(1, HKV, D)
    v_deq = ops.dequantize_kv(*ops.quantize_kv(v_plain.cpu())).to(DEV)
    got = y.view(HKV, hq // HKV, D)
    assert torch.equal(got, v_deq[0][:, None, :].expand_as(got))
    assert not torch.equal(v_deq, v_plain)
    _, v_cached = ref.gather_kv(f8[0].cpu(), f8[1].cpu(), bt[0].cpu(), 1, f8[2].cpu())
    assert torch.equal(v_cached, v_deq.cpu()), "the cache holds the token as it was folded"
    assert int((f8[2] != SENT_SCALE).sum()) == 2 * HKV, "one K and one V scale per kv head, nothing else"


def test_fused_decode_in_launch_merge_equals_the_reduce_launch(filled):
    hq, nslabs, B = 32, 2, 4
    ws = ops.decode_workspace(B, hq, D, device=DEV, Hkv=HKV)
    ws_sep = (torch.empty_like(ws[0]), torch.empty_like(ws[1]))
    cs = ref.rope_cos_sin(4096, D, 500000.0, None, device=DEV)
    for it, lens in enumerate([[1800, 5, 300, 2300], [40, 1999, 1, 257]]):
        bt, lens_t, pos, slots, slabs = _fused_inputs(lens, hq, nslabs, 50 + it, filled["nb"])
        a = tuple(t.clone() for t in filled["f8"])
        b = tuple(t.clone() for t in filled["f8"])
        y = ops.paged_decode_fused(slabs.reshape(-1), nslabs, pos, cs, slots, a[0], a[1], bt, lens_t, hq, HKV, D,
                                   SCALE, workspace=ws, splits=16, kv_scale=a[2])
        r = ops.paged_decode_fused(slabs.reshape(-1), nslabs, pos, cs, slots, b[0], b[1], bt, lens_t, hq, HKV, D,
                                   SCALE, workspace=ws_sep, splits=16, kv_scale=b[2])
        torch.cuda.synchronize()
        assert torch.equal(y, r), f"launch {it}: merge != reduce launch"
        assert int(ws[2].abs().sum()) == 0, f"launch {it}: counters not reset"


# ------------------------------------------------------------------ prefill
@pytest.mark.parametrize("hq", [8, 32])
@pytest.mark.parametrize("ctx,new", [(0, 40), (16, 1), (100, 130), (257, 64)])
def test_prefill_reads_the_prefix_dequantised_and_its_own_tokens_unquantised(ctx, new, hq):
    """Hq/Hkv 8/8 (bf16 routes to v1 as well): bit-identical to the bf16 v1 kernel over the
    dequantised prefix.  32/8: within 2e-2 of the bf16 v2 kernel over a bf16 cache of [dequantised
    prefix | unquantised new tokens], and of the fp32 reference."""
    nb = (ctx + new + BS - 1) // BS + 3
    g = torch.Generator(device="cpu").manual_seed(ctx + new)
    bt = _tables(1, nb - 2, nb, ctx)
    k = torch.randn(ctx + new, HKV, D, generator=g).to(torch.bfloat16)
    v = (torch.randn(ctx + new, HKV, D, generator=g) * 2).to(torch.bfloat16)
    q = torch.randn(new, hq, D, generator=g).to(torch.bfloat16)
    qkv = torch.cat([q.reshape(new, -1), k[ctx:].reshape(new, -1), v[ctx:].reshape(new, -1)], dim=1).contiguous().to(DEV)
    k8, v8, sc = (t[0] for t in ops.kv_cache_alloc(1, nb, HKV, D, F8, "cpu"))
    kd, vd = (t[0] for t in ops.kv_cache_alloc(1, nb, HKV, D, torch.bfloat16, "cpu"))
    s_all = _slots(bt[0].cpu(), 0, ctx + new)
    ref.write_kv_cache(k, v, k8, v8, s_all, sc)  # the engine writes the new tokens (quantised) before attending
    dq = lambda x: ops.dequantize_kv(*ops.quantize_kv(x))  # noqa: E731
    ref.write_kv_cache(torch.cat([dq(k[:ctx]), k[ctx:]]), torch.cat([dq(v[:ctx]), v[ctx:]]), kd, vd, s_all)
    cu = torch.tensor([0, new], dtype=torch.int32, device=DEV)
    cst = torch.tensor([ctx], dtype=torch.int32, device=DEV)
    y = ops.flash_prefill(qkv, cu, hq, HKV, D, SCALE, paged=(cst, k8.to(DEV), v8.to(DEV), bt), kv_scale=sc.to(DEV))
    r = ops.flash_prefill(qkv, cu, hq, HKV, D, SCALE, paged=(cst, kd.to(DEV), vd.to(DEV), bt))
    torch.cuda.synchronize()
    if hq == HKV:
        assert torch.equal(y, r), f"{int((y != r).sum())} of {y.numel()} outputs differ from bf16 v1"
    else:
        _close(y, r, "fp8 v1 vs bf16 v2")
    rr = ref.paged_prefill(qkv.cpu(), cu.cpu(), cst.cpu(), k8, v8, bt.cpu(), hq, HKV, D, SCALE, kv_scale=sc)
    _close(y.cpu(), rr, "fp8 prefill vs fp32 reference")


def test_engine_refuses_fp8_on_the_gpu_for_head_dim_64():
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine
    from k8s_llm_monitor_amd.models import get_config

    assert get_config("llama-tiny").head_dim != 128
    with pytest.raises(ValueError, match="head_dim 128"):
        LLMEngine(EngineConfig(model="llama-tiny", max_num_seqs=2, max_model_len=64, num_blocks=8, use_graphs=False,
                               kv_cache_dtype="fp8"), device="cuda")
