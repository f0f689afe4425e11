"""The fp8 (e4m3) KV cache on the CPU: the format (ops.quantize_kv), the reference write / gather
over an fp8 cache, the prefill rule (this step's own tokens are attended unquantised, only the
cached prefix dequantised) and a CPU engine running on it."""
import math

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.ops import cpu_attn
from k8s_llm_monitor_amd.ops import reference as ref

F8 = torch.float8_e4m3fn


# ------------------------------------------------------------------ format
def _vectors():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 4, 64, generator=g)
    x[1] *= 1e-3
    x[2] *= 300.0
    x[3, 0] = 0.0  # an all-zero vector
    x[4, 1] = 0.0
    x[4, 1, 7] = 448.0  # amax / 448 exactly 1: the upper end of (224, 448]
    x[5, 2, 3] = 2.0 ** -80  # with the rest zero the exponent clamps at -60
    x[5, 2, :3] = 0.0
    x[5, 2, 4:] = 0.0
    return x.to(torch.bfloat16)


def test_scale_is_a_power_of_two_with_amax_in_the_top_binade():
    x = _vectors()
    q, s = ops.quantize_kv(x)
    assert q.dtype == F8 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == x.shape[:2]
    m, _ = torch.frexp(s)
    assert torch.all(m == 0.5), "every scale is 2^e"
    amax = x.float().abs().amax(-1)
    live = (amax > 2.0 ** -50)
    r = amax[live] / s[live]
    assert torch.all(r > 224) and torch.all(r <= 448)
    assert float(s[4, 1]) == 1.0 and float(s[3, 0]) == 1.0
    assert torch.all(q[3, 0].float() == 0), "all-zero vector: scale 1, codes 0"
    assert float(s[5, 2]) == 2.0 ** -60, "the exponent is clamped to [-60, 60]"
    assert not torch.isnan(q.float()).any()


def test_dequantised_values_are_exact_in_bf16_and_requantise_to_the_same_codes():
    x = _vectors()
    q, s = ops.quantize_kv(x)
    d32 = q.float() * s[..., None]
    d = ops.dequantize_kv(q, s)
    assert d.dtype == torch.bfloat16 and torch.equal(d.float(), d32)
    # quantising the dequantised values again changes no value.  Codes and scales repeat as well,
    # except where the vector's amax rounded DOWN to 224 x scale (amax / scale in (224, 232)): 224 is
    # the open lower end of the rule's (224, 448], so the second pass picks half the scale and twice
    # the codes - the same numbers
    q2, s2 = ops.quantize_kv(d)
    assert torch.equal(ops.dequantize_kv(q2, s2), d)
    same = q.float().abs().amax(-1) > 224
    assert int(same.sum()) > 100 and int((~same).sum()) > 0
    assert torch.equal(q2.view(torch.uint8)[same], q.view(torch.uint8)[same]) and torch.equal(s2[same], s[same])
    halved = ~same & (s > 2.0 ** -60) & (q.float().abs().amax(-1) > 0)
    assert torch.equal(s2[halved] * 2, s[halved])
    # the quantisation error is within half an e4m3 step of the scaled value (3 mantissa bits)
    err = (d32 - x.float()).abs()
    assert torch.all(err <= x.float().abs() * 2.0 ** -4 + s[..., None] * 2.0 ** -10)


def test_alloc_owns_the_layout_and_the_byte_count():
    k, v, sc = ops.kv_cache_alloc(2, 5, 4, 64, F8, "cpu")
    assert k.shape == (2, 5, 4, 8, 16, 8) and v.shape == (2, 5, 4, 64, 16) and sc.shape == (2, 5, 4, 2, 16)
    assert k.dtype == v.dtype == F8 and sc.dtype == torch.float32
    kb, vb = ops.kv_cache_alloc(2, 5, 4, 64, torch.bfloat16, "cpu")
    assert kb.shape == k.shape and vb.shape == v.shape and kb.dtype == torch.bfloat16
    n8 = ops.kv_bytes_per_block(2, 4, 64, F8)
    assert n8 * 5 == k.numel() + v.numel() + 4 * sc.numel()
    assert ops.kv_bytes_per_block(2, 4, 64, torch.bfloat16) * 5 == 2 * (kb.numel() + vb.numel())
    assert ops.kv_bytes_per_block(32, 8, 128, torch.bfloat16) / ops.kv_bytes_per_block(32, 8, 128, F8) > 1.93


# ------------------------------------------------------------------ reference write / gather
SENT_CODE, SENT_SCALE = 0x5A, 7.0


def _sentinel_cache(nb, hkv, D):
    k, v, sc = (t[0] for t in ops.kv_cache_alloc(1, nb, hkv, D, F8, "cpu"))
    k.view(torch.uint8).fill_(SENT_CODE)
    v.view(torch.uint8).fill_(SENT_CODE)
    sc.fill_(SENT_SCALE)
    return k, v, sc


def test_write_then_gather_round_trips_and_leaves_other_slots_alone():
    hkv, D, nb = 2, 64, 8
    g = torch.Generator().manual_seed(1)
    k_cache, v_cache, sc = _sentinel_cache(nb, hkv, D)
    bt = torch.tensor([5, 2, 7, 0], dtype=torch.int32)
    n0, n = 11, 30  # the sequence's tokens 11 .. 40: starts mid-block, crosses two block ends
    kx = torch.randn(n, hkv, D, generator=g).to(torch.bfloat16)
    vx = (torch.randn(n, hkv, D, generator=g) * 5).to(torch.bfloat16)
    pos = torch.arange(n0, n0 + n)
    slots = (bt[pos // 16].long() * 16 + pos % 16).to(torch.int32)
    slots_in = torch.cat([slots[:7], torch.tensor([-1], dtype=torch.int32), slots[7:]])  # a -1 slot writes nothing
    kin = torch.cat([kx[:7], kx[:1], kx[7:]])
    vin = torch.cat([vx[:7], vx[:1], vx[7:]])
    ref.write_kv_cache(kin, vin, k_cache, v_cache, slots_in, sc)
    k, v = ref.gather_kv(k_cache, v_cache, bt, n0 + n, sc)
    assert torch.equal(k[n0:].float(), ops.dequantize_kv(*ops.quantize_kv(kx)).float())
    assert torch.equal(v[n0:].float(), ops.dequantize_kv(*ops.quantize_kv(vx)).float())
    kb, vb = cpu_attn.gather_batch(k_cache, v_cache, bt[None], 3, sc)
    assert torch.equal(kb[0, :, n0:n0 + n].transpose(0, 1), k[n0:].float())
    assert torch.equal(vb[0, :, n0:n0 + n].transpose(0, 1), v[n0:].float())
    # everything outside the written tokens still holds the sentinels
    written = torch.zeros(nb * 16, dtype=torch.bool)
    written[slots.long()] = True
    w = written.view(nb, 16)
    ku, vu = k_cache.view(torch.uint8), v_cache.view(torch.uint8)
    assert torch.all(ku.permute(0, 3, 1, 2, 4)[~w] == SENT_CODE)
    vseq = vu[..., ref.v_perm(torch.arange(16))]  # tokens in sequence order
    assert torch.all(vseq.permute(0, 3, 1, 2)[~w] == SENT_CODE)
    assert torch.all(sc.permute(0, 3, 1, 2)[~w] == SENT_SCALE)
    assert torch.all(sc.permute(0, 3, 1, 2)[w] != SENT_SCALE)


# ------------------------------------------------------------------ prefill: in-step tokens unquantised
@pytest.mark.parametrize("impl", ["cpu_attn", "reference"])
def test_paged_prefill_attends_its_own_tokens_unquantised(impl):
    Hq, Hkv, D, nb = 4, 2, 64, 16
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(2)
    ctxs, news = [21, 16], [13, 5]
    k_cache, v_cache, sc = (t[0] for t in ops.kv_cache_alloc(1, nb, Hkv, D, F8, "cpu"))
    perm = torch.randperm(nb, generator=g).to(torch.int32)
    bt = perm[:6].view(2, 3)
    rows, full_k, full_v = [], [], []
    for i, (c, n) in enumerate(zip(ctxs, news)):
        kx = torch.randn(c + n, Hkv, D, generator=g).to(torch.bfloat16)
        vx = (torch.randn(c + n, Hkv, D, generator=g) * 3).to(torch.bfloat16)
        pos = torch.arange(c + n)
        slots = (bt[i][pos // 16].long() * 16 + pos % 16).to(torch.int32)
        ref.write_kv_cache(kx, vx, k_cache, v_cache, slots, sc)  # prefix and (as the engine does) the new tokens
        q = torch.randn(n, Hq, D, generator=g).to(torch.bfloat16)
        rows.append(torch.cat([q.reshape(n, -1), kx[c:].reshape(n, -1), vx[c:].reshape(n, -1)], dim=1))
        full_k.append(kx)
        full_v.append(vx)
    qkv = torch.cat(rows)
    cu = torch.tensor([0, news[0], news[0] + news[1]], dtype=torch.int32)
    cs = torch.tensor(ctxs, dtype=torch.int32)
    fn = cpu_attn.paged_prefill if impl == "cpu_attn" else ref.paged_prefill
    out = fn(qkv, cu, cs, k_cache, v_cache, bt, Hq, Hkv, D, scale, kv_scale=sc).float()
    via_ops = ops.flash_prefill(qkv, cu, Hq, Hkv, D, scale, paged=(cs, k_cache, v_cache, bt), kv_scale=sc).float()
    a = 0
    for i, (c, n) in enumerate(zip(ctxs, news)):
        dq = lambda x: ops.dequantize_kv(*ops.quantize_kv(x)).float()  # noqa: E731
        q = qkv[a:a + n, : Hq * D].view(n, Hq, D)
        mixed = ref.attention(q, torch.cat([dq(full_k[i][:c]), full_k[i][c:].float()]),
                              torch.cat([dq(full_v[i][:c]), full_v[i][c:].float()]), scale, causal=True).reshape(n, -1)
        allq = ref.attention(q, dq(full_k[i]), dq(full_v[i]), scale, causal=True).reshape(n, -1)
        tol = 2.0 ** -8 * float(mixed.abs().max())  # the bf16 rounding of the output
        assert float((out[a:a + n] - mixed).abs().max()) <= tol
        assert float((via_ops[a:a + n] - mixed).abs().max()) <= tol
        assert float((out[a:a + n] - allq).abs().max()) > 4 * tol, "the in-step tokens were read from the cache"
        a += n


def test_cpu_paged_decode_reads_the_dequantised_cache():
    Hq, Hkv, D, nb = 4, 2, 64, 8
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(3)
    k_cache, v_cache, sc = (t[0] for t in ops.kv_cache_alloc(1, nb, Hkv, D, F8, "cpu"))
    lens = [1, 17, 40]
    bt = torch.tensor([[3, 0, 0], [1, 6, 0], [7, 2, 5]], dtype=torch.int32)
    kd, vd = torch.zeros_like(k_cache, dtype=torch.bfloat16), torch.zeros_like(v_cache, dtype=torch.bfloat16)
    for i, n in enumerate(lens):
        kx = torch.randn(n, Hkv, D, generator=g).to(torch.bfloat16)
        vx = torch.randn(n, Hkv, D, generator=g).to(torch.bfloat16)
        pos = torch.arange(n)
        slots = (bt[i][pos // 16].long() * 16 + pos % 16).to(torch.int32)
        ref.write_kv_cache(kx, vx, k_cache, v_cache, slots, sc)
        ref.write_kv_cache(ops.dequantize_kv(*ops.quantize_kv(kx)), ops.dequantize_kv(*ops.quantize_kv(vx)), kd, vd, slots)
    q = torch.randn(3, Hq * D, generator=g).to(torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32)
    got = ops.paged_decode(q, k_cache, v_cache, bt, sl, Hq, Hkv, D, scale, kv_scale=sc)
    want = ops.paged_decode(q, kd, vd, bt, sl, Hq, Hkv, D, scale)
    assert torch.equal(got, want)
    assert torch.equal(ref.paged_decode(q, k_cache, v_cache, bt, sl, Hq, Hkv, D, scale, kv_scale=sc),
                       ref.paged_decode(q, kd, vd, bt, sl, Hq, Hkv, D, scale))


# ------------------------------------------------------------------ engine
def _engine(**kw):
    return LLMEngine(EngineConfig(model="llama-tiny", max_num_seqs=4, max_model_len=256, use_graphs=False,
                                  dtype="float32", prefix_caching=True, chunked_prefill=True, max_prefill_tokens=32,
                                  seed=3, **kw), device="cpu")


def test_cpu_engine_generates_on_an_fp8_cache_with_prefix_caching_and_chunked_prefill():
    eng = _engine(kv_cache_dtype="fp8", kv_cache_gb=0.01)
    sp = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    shared = "cluster overview: node-001 CPU=93% memory pressure; node-002 NotReady; " * 2
    first = eng.generate([shared + "why does my pod restart?"], sp)
    again = eng.generate([shared + "why does my pod restart?", shared + "which node is unhealthy?"], sp)
    assert all(len(s.output_ids) == 6 for s in first + again)
    assert len(first[0].prompt_ids) > 32, "the prompt is longer than one prefill chunk"
    assert again[0].output_ids == first[0].output_ids
    st = eng.stats()
    assert st["kv_cache_dtype"] == "fp8"
    r = eng.runner
    assert r.k_cache.dtype == F8 and r.kv_scale is not None and len(r.kv[0]) == 3 and r.kv[0][2] is not None
    assert float(r.kv_scale.abs().max()) > 0, "scales were written"
    assert st["kv_cache_bytes"] == r.k_cache.numel() + r.v_cache.numel() + 4 * r.kv_scale.numel()
    assert r.kv_stats()["kv_cache_dtype"] == "fp8"
    plain = _engine(kv_cache_gb=0.01)
    ps = plain.stats()
    assert ps["kv_cache_dtype"] == "bf16" and plain.runner.kv[0][2] is None
    assert st["kv_blocks"] >= 1.9 * ps["kv_blocks"], (st["kv_blocks"], ps["kv_blocks"])
    assert st["kv_blocks_total"] == st["kv_blocks"]


def test_default_is_bf16_and_other_values_are_refused():
    assert EngineConfig().kv_cache_dtype == "bf16"
    with pytest.raises(ValueError):
        _engine(kv_cache_dtype="int4", num_blocks=32)


def test_monitor_config_passes_kv_cache_dtype_on():
    from k8s_llm_monitor_amd.monitor.app import engine_config
    from k8s_llm_monitor_amd.monitor.config import from_dict

    assert engine_config(from_dict({})).kv_cache_dtype == "bf16"
    assert engine_config(from_dict({"llm": {"kv_cache_dtype": "fp8"}})).kv_cache_dtype == "fp8"
