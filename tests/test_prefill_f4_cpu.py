"""prefill_weights="mxfp4" on the CPU path: the mxfp4 codes and block scales as the ONLY resident
copy of a dense projection and of the LM head (the bf16 copy released), on top of
decode_weights="mxfp4".

The model is the one tests/test_prefill_f8_cpu.py uses - llama-tiny with 2 heads / 1 kv head of 128
and ffn 256 (d_model 256, vocab 512, 2 layers): the eligibility rule (an mxfp4 decode form in every
row class, ops.tile_f4_ok, dense, TP = 1, ONE_LAYOUT) selects all four projections and the head of
it too (test_the_config_is_the_rule_s_pick).  ONE_LAYOUT = "force" as in tests/test_one_layout.py."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.models import AttnMeta, CausalLM, get_config
from k8s_llm_monitor_amd.models.checkpoint import load_checkpoint, save_checkpoint
from k8s_llm_monitor_amd.models.llama import PROJ

CFG = get_config("llama-tiny").replace(n_heads=2, n_kv_heads=1, head_dim=128, ffn_dim=256)


@pytest.fixture(autouse=True)
def _one_layout(monkeypatch):
    monkeypatch.setattr(CausalLM, "ONE_LAYOUT", "force")


def _model(seed=5, cfg=CFG, **kw):
    kw.setdefault("dec_weights", "mxfp4")
    return CausalLM(cfg, device="cpu", seed=seed, **kw)


def _only(**kw):
    kw.setdefault("prefill_weights", "mxfp4")
    return _model(**kw)


def _dq(w, scale):
    """The values of a packed mxfp4 encoding (what every kernel computes with)."""
    return ops.dequantize_mxfp4(*ops.unpack_skinny_f4(w, scale))


def _assert_codes_only(m):
    assert set(m.prefill_encodings().values()) == {"mxfp4"}, m.prefill_encodings()
    assert set(m.decode_encodings().values()) == {"mxfp4"}
    for L in m.layers:
        for key in PROJ:
            assert ops.is_mxfp4(L[key]) and L[key] is L[key + "_q"] and L[key + "_qs"].dtype == torch.uint8
            assert not any(key + sfx in L for sfx in ("_d", "_p", "_dg", "_pg")), sorted(L)
        big = [k for k, v in L.items() if torch.is_tensor(v) and v.dim() >= 2 and v.dtype != torch.uint8]
        assert not big, f"a bf16 matrix is still resident: {big}"
    assert m.lm_head is m.lm_head_q and ops.is_mxfp4(m.lm_head) and m.lm_head_d is None


def test_the_config_is_the_rule_s_pick():
    c = CFG
    nq, no, d, f = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, c.n_heads * c.head_dim, c.d_model, c.ffn_dim
    for N, K, epi in ((nq, d, 0), (d, no, 0), (2 * f, d, 2), (d, f, 0), (c.vocab_size, d, 1)):
        assert ops.tile_f4_ok(N, K)
        assert all(ops.dec_config(N, K, epi, rows=r, f4=True) is not None for r in ops.dec_row_classes())
    # tile_f4_ok's boundaries: whole 16-row blocks, whole 128-deep scale groups, at least two of them
    assert ops.tile_f4_ok(16, 256) and ops.tile_f4_ok(16, 384)
    assert not ops.tile_f4_ok(16, 128) and not ops.tile_f4_ok(8, 256)
    assert not ops.tile_f4_ok(16, 320) and not ops.tile_f4_ok(16, 192) and not ops.tile_f4_ok(24, 256)
    # 2^31 bytes of codes: past the 32-bit DMA offsets; one block row less fits
    assert not ops.tile_f4_ok(1 << 16, 1 << 16) and ops.tile_f4_ok((1 << 16) - 16, 1 << 16)


def test_codes_only_model_holds_no_bf16_projection_and_counts_to_the_byte():
    m = _only()
    _assert_codes_only(m)
    assert m._packed and m.dec_rows_max() == ops.DEC_MAX_M and m._rc_o == 0
    c = m.cfg
    nq, no, d, f = (m.hq + 2 * m.hkv) * m.D, m.hq * m.D, c.d_model, c.ffn_dim
    # half a byte per code, one scale byte per 32
    per_layer = sum(N * K // 2 + N * K // 32 for N, K in ((nq, d), (d, no), (2 * f, d), (d, f))) + 2 * 2 * d
    want = c.n_layers * per_layer + (c.vocab_size * d // 2 + c.vocab_size * d // 32) + 2 * c.vocab_size * d + 2 * d
    assert m.resident_weight_bytes() == want
    both = _model()
    # a code tensor holds two elements per byte: the bf16 copy released is 2 bytes x 2 x numel
    released = sum(4 * L[k + "_q"].numel() for L in both.layers for k in PROJ) + 4 * both.lm_head_q.numel()
    assert both.resident_weight_bytes() - m.resident_weight_bytes() == released
    assert m.num_local_params() == both.num_local_params()
    assert set(both.prefill_encodings().values()) == {"bf16"}


def _run(m):
    """Prefill of two prompts (5 and 9 tokens) and one decode step; returns (logits, logits, kv)."""
    bs, nb = 16, 8
    g = torch.Generator().manual_seed(0)
    kv = [(torch.randn(nb, m.hkv, m.D // 8, bs, 8, generator=g).to(m.dtype),
           torch.randn(nb, m.hkv, m.D, bs, generator=g).to(m.dtype)) for _ in m.layers]
    ids = torch.randint(0, 500, (14,), generator=g, dtype=torch.int32)
    pos = torch.cat([torch.arange(5), torch.arange(9)]).to(torch.int32)
    slots = torch.cat([torch.arange(5), 16 + torch.arange(9)]).to(torch.int32)
    meta = AttnMeta(is_prefill=True, positions=pos, slot_mapping=slots,
                    cu_seqlens=torch.tensor([0, 5, 14], dtype=torch.int32), logits_idx=torch.tensor([4, 13]))
    a = m.forward(ids, meta, kv)
    lens = torch.tensor([6, 10])
    dm = AttnMeta(is_prefill=False, positions=(lens - 1).to(torch.int32),
                  slot_mapping=torch.tensor([5, 25], dtype=torch.int32),
                  block_tables=torch.tensor([[0, 3], [1, 2]], dtype=torch.int32), seq_lens=lens.to(torch.int32))
    b = m.forward(torch.tensor([7, 99], dtype=torch.int32), dm, kv)
    return a, b, kv


def test_codes_only_equals_the_two_copy_mxfp4_model():
    only, both = _only(), _model()
    for La, Lb in zip(only.layers, both.layers):
        for key in PROJ:
            assert torch.equal(only.canonical(La, key), both.canonical(Lb, key)), key
            assert torch.equal(La[key + "_q"], Lb[key + "_q"]) and torch.equal(La[key + "_qs"], Lb[key + "_qs"])
    assert torch.equal(only.canonical_head(), both.canonical_head())
    (pa, da, kva), (pb, db, kvb) = _run(only), _run(both)
    assert torch.isfinite(pa).all() and torch.equal(pa, pb), "prefill logits"
    assert torch.isfinite(da).all() and torch.equal(da, db), "decode logits"
    for (ka, va), (kb, vb) in zip(kva, kvb):
        assert torch.equal(ka, kb) and torch.equal(va, vb)


def test_checkpoint_round_trip_into_a_codes_only_model(tmp_path):
    src = _only()
    save_checkpoint(src, tmp_path / "ckpt")
    dst = _only(seed=9)
    assert not torch.equal(dst.canonical(dst.layers[0], "wo"), src.canonical(src.layers[0], "wo"))
    load_checkpoint(dst, tmp_path / "ckpt")
    _assert_codes_only(dst)
    for La, Lb in zip(src.layers, dst.layers):
        for key in PROJ:
            assert torch.equal(_dq(La[key], La[key + "_qs"]), _dq(Lb[key], Lb[key + "_qs"])), key
    assert torch.equal(src.canonical_head(), dst.canonical_head())
    assert torch.equal(_run(src)[0], _run(dst)[0])
    empty = _only(init="empty")  # what the engine builds before a load: nothing quantised yet
    assert set(empty.prefill_encodings().values()) == {"bf16"}
    load_checkpoint(empty, tmp_path / "ckpt")
    _assert_codes_only(empty)
    assert torch.equal(_run(src)[0], _run(empty)[0])


def test_copy_weights_from_in_both_directions(monkeypatch):
    only = _only()
    # out of a codes-only model: the fp32 reference gets the dequantised values
    monkeypatch.setattr(CausalLM, "ONE_LAYOUT", False)
    ref32 = CausalLM(CFG, device="cpu", dtype=torch.float32, seed=1)
    ref32.copy_weights_from(only)
    monkeypatch.setattr(CausalLM, "ONE_LAYOUT", "force")
    for La, Lb in zip(only.layers, ref32.layers):
        for key in PROJ:
            assert torch.equal(only.canonical(La, key).float(), ref32.canonical(Lb, key)), key
    assert torch.equal(only.canonical_head().float(), ref32.canonical_head())
    # into one: requantised from the source's values, still codes-only
    src = _model(seed=21, dec_weights="bf16")
    only.copy_weights_from(src)
    _assert_codes_only(only)
    for La, Lb in zip(only.layers, src.layers):
        for key in PROJ:
            q, s = ops.quantize_mxfp4(src.canonical(Lb, key))
            assert torch.equal(only.canonical(La, key), ops.dequantize_mxfp4(q, s)), key
    q, s = ops.quantize_mxfp4(src.canonical_head())
    assert torch.equal(only.canonical_head(), ops.dequantize_mxfp4(q, s))
    # values already of the form code * 2^e requantise to themselves
    again = _only(seed=33)
    again.copy_weights_from(only)
    for La, Lb in zip(only.layers, again.layers):
        for key in PROJ:
            assert torch.equal(_dq(La[key], La[key + "_qs"]), _dq(Lb[key], Lb[key + "_qs"])), key
    assert torch.equal(_run(only)[0], _run(again)[0])


def test_init_skinny_twice_keeps_values_and_stays_within_one_layer(monkeypatch):
    m = _only(cfg=CFG.replace(n_layers=6))  # six layers: one layer's bf16 is far from the whole model's
    vals = [{k: _dq(L[k], L[k + "_qs"]) for k in PROJ} for L in m.layers]
    head = m.canonical_head()
    before = m.resident_weight_bytes()
    L0 = m.layers[0]
    layer_bf16 = sum(4 * L0[k].numel() for k in PROJ)  # two codes per byte, two bytes per bf16
    head_bf16 = 4 * m.lm_head.numel()
    seen = []
    real = ops.quantize_mxfp4
    monkeypatch.setattr(ops, "quantize_mxfp4", lambda w: (seen.append(m.resident_weight_bytes()), real(w))[1])
    m._init_skinny()
    monkeypatch.setattr(ops, "quantize_mxfp4", real)
    # bf16 comes back one layer at a time - that layer's row-major tensors and their packed copies -
    # plus the head, which is turned back first: never the six layers' 6 x layer_bf16
    assert seen and max(seen) <= before + 2 * layer_bf16 + head_bf16, (max(seen), before, layer_bf16, head_bf16)
    assert 2 * layer_bf16 + head_bf16 < 3 * layer_bf16
    _assert_codes_only(m)
    assert m.resident_weight_bytes() == before
    for L, v in zip(m.layers, vals):
        for k in PROJ:
            assert torch.equal(_dq(L[k], L[k + "_qs"]), v[k]), k
    assert torch.equal(m.canonical_head(), head)


def test_errors_and_fallbacks(caplog):
    with pytest.raises(ValueError, match="decode weights"):
        _model(dec_weights="bf16", prefill_weights="mxfp4")
    with pytest.raises(ValueError, match="decode weights"):
        _model(dec_weights="fp8", prefill_weights="mxfp4")
    with pytest.raises(ValueError, match="decode weights"):
        _model(dec_weights="mxfp4", prefill_weights="fp8")
    with pytest.raises(ValueError, match="prefill weights"):
        _only(prefill_weights="int4")
    assert CausalLM.PREFILL_WEIGHTS == "bf16"
    m = _only()
    with pytest.raises(ValueError, match="row-complete"):
        m.set_decode_fusion(rc=True)
    m.set_decode_fusion()
    m.set_decode_fusion(rc=False)
    assert m._rc_o == 0
    # d_model 128: K = 128 has no mxfp4 form of the tile GEMM (and the model is not ONE_LAYOUT):
    # it builds, keeps both copies and says so
    with caplog.at_level("INFO"):
        tiny = _only(cfg=get_config("llama-tiny").replace(d_model=128))
    assert set(tiny.prefill_encodings().values()) == {"bf16"}
    assert any("prefill_weights=mxfp4 keeps the bf16 copy" in r.getMessage() for r in caplog.records)
    two = _model(cfg=tiny.cfg)
    assert tiny.resident_weight_bytes() == two.resident_weight_bytes()
    assert torch.equal(_run(tiny)[0], _run(two)[0])


def test_an_moe_model_keeps_both_copies_and_says_why(caplog):
    cfg = get_config("mixtral-tiny")
    with caplog.at_level("INFO"):
        moe = _only(cfg=cfg)
    assert set(moe.prefill_encodings().values()) == {"bf16"}
    msgs = [r.getMessage() for r in caplog.records if "keeps the bf16 copy" in r.getMessage()]
    assert msgs and "MoE" in msgs[0] and "prefill_weights=mxfp4" in msgs[0], msgs
    assert moe.resident_weight_bytes() == _model(cfg=cfg).resident_weight_bytes()


def test_tied_head_keeps_the_embedding_and_drops_only_the_decode_copy():
    cfg = CFG.replace(tie_embeddings=True)
    m, both = _only(cfg=cfg), _model(cfg=cfg)
    assert m.lm_head is m.embed and m.embed.dtype == torch.bfloat16
    assert m.lm_head_d is None and m.lm_head_q is not None and m.prefill_encodings()["head"] == "mxfp4"
    assert both.resident_weight_bytes() - m.resident_weight_bytes() == (
        sum(4 * L[k + "_q"].numel() for L in both.layers for k in PROJ) + 4 * both.lm_head_q.numel())
    (pa, da, _), (pb, db, _) = _run(m), _run(both)
    assert torch.equal(da, db) and torch.equal(pa, pb)


def test_engine_stats_and_config_plumbing():
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from k8s_llm_monitor_amd.monitor.app import engine_config
    from k8s_llm_monitor_amd.monitor.config import from_dict

    ec = engine_config(from_dict({"llm": {"decode_weights": "mxfp4", "prefill_weights": "mxfp4"}}))
    assert ec.prefill_weights == "mxfp4" and ec.decode_weights == "mxfp4"
    kw = dict(model="llama-tiny", model_overrides=dict(n_heads=2, n_kv_heads=1, head_dim=128, ffn_dim=256),
              max_num_seqs=4, max_model_len=256, num_blocks=64, use_graphs=False, prefix_caching=False, seed=3)
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(prefill_weights="mxfp4", **kw), device="cpu")
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(decode_weights="fp8", prefill_weights="mxfp4", **kw), device="cpu")
    eng = LLMEngine(EngineConfig(decode_weights="mxfp4", prefill_weights="mxfp4", **kw), device="cpu")
    st = eng.stats()
    assert st["prefill_weights"] == "mxfp4" and set(st["prefill_encodings"].values()) == {"mxfp4"}
    assert st["resident_weight_bytes"] == eng.model.resident_weight_bytes()
    two = LLMEngine(EngineConfig(decode_weights="mxfp4", **kw), device="cpu")
    assert two.stats()["prefill_weights"] == "bf16" and set(two.stats()["prefill_encodings"].values()) == {"bf16"}
    assert two.stats()["resident_weight_bytes"] > st["resident_weight_bytes"]
    sp = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    prompts = ["pod crashloop in kube-system", "node-003 NotReady"]
    assert [s.output_ids for s in eng.generate(prompts, sp)] == [s.output_ids for s in two.generate(prompts, sp)]


# ------------------------------------------------------------------ the CPU reference of gemm_tile
def _quant(w):
    q, s = ops.quantize_mxfp4(w)
    return (ops.dequantize_mxfp4(q, s),) + ops.pack_skinny_f4(q, s)


@pytest.mark.parametrize("epi", ["plain", "swiglu8", "rope", "swiglu8_rs", "rope_rs", "resid"])
def test_gemm_tile_cpu_mxfp4_equals_bf16_over_dequantised(epi):
    from k8s_llm_monitor_amd.ops import reference as ref

    M, N, K = 37, 256, 512
    g = torch.Generator().manual_seed(4)
    w = torch.randn(N, K, generator=g) * 0.02 * torch.exp2((torch.arange(N) % 7 - 3).float())[:, None]
    w = (w * torch.exp2((torch.arange(K // 32) % 3 - 2).float()).repeat_interleave(32)[None, :]).to(torch.bfloat16)
    w[5] = 0
    if epi.startswith("swiglu8"):
        w = ops.interleave_gate_up8(w).contiguous()
    dq, qp, s = _quant(w)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    kw = {}
    if epi.startswith("swiglu8"):
        kw["swiglu"] = 8
    if epi.startswith("rope"):
        kw["rope"] = ((torch.arange(M) * 5 % 64).to(torch.int32), ref.rope_cos_sin(64, 128, 10000.0).float(), 1)
    if epi.endswith("_rs"):
        kw["rowscale"] = (torch.rand(M, K // 128, generator=g) * 64 + 16, 1e-5)
    if epi == "resid":
        r = torch.randn(M, N, generator=g).to(torch.bfloat16)
        nw = (torch.rand(N, generator=g) + 0.5).to(torch.bfloat16)
        outs = []
        for wgt, k2 in ((qp, dict(wscale=s)), (ops.pack_skinny(dq), {}), (dq, {})):
            rr = r.clone()
            hw, ss = ops.gemm_tile_resid(x, wgt, rr, nw, **k2)
            outs.append((rr, hw, ss))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], o))
        return
    y4 = ops.gemm_tile(x, qp, algo=1, wscale=s, **kw)
    assert torch.equal(y4, ops.gemm_tile(x, ops.pack_skinny(dq), algo=1, **kw))
    assert torch.equal(y4, ops.gemm_tile(x, dq, algo=1, **kw))
    if epi in ("plain", "swiglu8"):
        assert torch.equal(y4, ops.prefill_linear(x, qp, swiglu=kw.get("swiglu", False), wscale=s))


def test_gemm_tile_cpu_mxfp4_unsupported_forms_raise():
    dq, qp, s = _quant((torch.randn(256, 256) * 0.02).to(torch.bfloat16))
    x = torch.randn(8, 256).to(torch.bfloat16)
    with pytest.raises(ValueError, match="schedule"):
        ops.gemm_tile(x, qp, algo=0, wscale=s)
    with pytest.raises(ValueError, match="grouped"):
        ops.gemm_tile(x, qp[None], torch.tensor([0, 8], dtype=torch.int32), algo=1, wscale=s)
    with pytest.raises(ValueError, match="swiglu=1"):
        ops.gemm_tile(x, qp, swiglu=True, algo=1, wscale=s)
    with pytest.raises(ValueError, match="scale"):
        ops.gemm_tile(x, qp, algo=1)
    with pytest.raises(ValueError, match="scale"):
        ops.gemm_tile(x, qp, algo=1, wscale=s.reshape(16, 2, 64))
    with pytest.raises(ValueError, match="scale"):
        ops.gemm_tile(x, qp, algo=1, wscale=s.float())
    with pytest.raises(ValueError, match="scale"):
        ops.gemm_tile_resid(x, qp, torch.zeros(8, 256).to(torch.bfloat16), torch.ones(256).to(torch.bfloat16))
    _, qp128, s128 = _quant((torch.randn(256, 128) * 0.02).to(torch.bfloat16))
    with pytest.raises(ValueError, match="K=128"):
        ops.gemm_tile(x[:, :128].contiguous(), qp128, algo=1, wscale=s128)
    assert ops.w_out(qp) == 256 and ops.w_in(qp) == 256 and ops.skinny_wdims(qp) == (256, 256)
