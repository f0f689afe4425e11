"""fp8 (e4m3) decode weights on the CPU path: the quantisation recipe, the packed layouts, the
reference form of ops.dec_gemm over an fp8 weight, the table of fp8 forms against the native
report, and an engine decoding from fp8 weights against a bf16-decoding one given its weights."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.models.checkpoint import load_checkpoint, save_checkpoint

F8 = torch.float8_e4m3fn


def _w(N, K, seed=0, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)


# ------------------------------------------------------------------ the recipe
@pytest.mark.parametrize("shape", [(272, 512), (64, 4096)])
def test_recipe_values_are_bf16_scales_powers_of_two_no_nan(shape):
    w = _w(*shape)
    q, s = ops.quantize_rows_fp8(w)
    assert q.dtype == F8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (shape[0],)
    m, _ = torch.frexp(s)
    assert torch.all(m == 0.5), "scales are powers of two"
    codes = q.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any(), "no NaN code"
    assert q.float().abs().max() <= 448
    # e = ceil(log2(amax / 448)): the row maximum lands in (224, 448]
    amax = w.float().abs().amax(1)
    assert torch.all(amax / s <= 448) and torch.all(amax / s > 224)
    dq32 = q.float() * s[:, None]
    dq = ops.dequantize_rows_fp8(q, s)
    assert dq.dtype == torch.bfloat16 and torch.equal(dq.float(), dq32), "dequantised values equal their bf16 rounding"
    assert torch.equal(q, (w.float() / s[:, None]).to(F8)), "codes round as Tensor.to(float8_e4m3fn)"
    # ordinary e4m3 rounding error on the product
    x = torch.randn(8, shape[1], generator=torch.Generator().manual_seed(1))
    ref = x @ w.float().t()
    rel = ((x @ dq32.t() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt().item()
    assert rel < 0.04, rel


def test_recipe_zero_row_and_single_max_rows():
    w = torch.zeros(16, 64)
    for r, k in enumerate((-20, -3, 0, 1, 9)):  # rows 0..4: a single 448 * 2^k value
        w[r, 3 * r] = 448.0 * 2.0 ** k
    w[5, 7] = -448.0 * 2.0 ** -5
    q, s = ops.quantize_rows_fp8(w.to(torch.bfloat16))
    assert torch.equal(s[:5], torch.tensor([2.0 ** k for k in (-20, -3, 0, 1, 9)]))
    assert torch.all(s[6:] == 1.0) and torch.all(q[6:].float() == 0), "an all-zero row: e = 0, codes 0"
    for r in range(5):
        assert q[r, 3 * r].float() == 448.0
    assert q[5, 7].float() == -448.0 and s[5] == 2.0 ** -5
    assert torch.equal(ops.dequantize_rows_fp8(q, s).float(), w)


def test_recipe_values_stable_under_requantisation():
    w = _w(272, 512, seed=3)
    w[0] = 0
    w[1, 5] = 3.0  # an outlier row
    q, s = ops.quantize_rows_fp8(w)
    dq = ops.dequantize_rows_fp8(q, s)
    q2, s2 = ops.quantize_rows_fp8(dq)
    assert torch.equal(ops.dequantize_rows_fp8(q2, s2), dq)


# ------------------------------------------------------------------ layouts
def test_pack_skinny_f8_round_trip_and_fragment_order():
    N, K = 48, 256
    q = torch.arange(N * K).reshape(N, K).remainder(251).to(torch.uint8).view(F8)
    p = ops.pack_skinny_f8(q)
    assert p.shape == (N // 16, K // 64, 64, 16) and p.dtype == F8 and p.is_contiguous()
    assert torch.equal(ops.unpack_skinny_f8(p).view(torch.uint8), q.view(torch.uint8))
    # lane l's 16 bytes: its 8 codes of k-step 2j, then its 8 of k-step 2j + 1, in pack_skinny's order
    b = q.view(torch.uint8).to(torch.int16)  # pack_skinny over a wider dtype holding the same numbers
    ps = ops.pack_skinny(b)  # [N/16, K/32, 64, 8]
    pu = p.view(torch.uint8).to(torch.int16)
    for j in range(K // 64):
        assert torch.equal(pu[:, j, :, :8], ps[:, 2 * j])
        assert torch.equal(pu[:, j, :, 8:], ps[:, 2 * j + 1])
    assert ops.skinny_wdims(p) == (N, K)
    with pytest.raises(ValueError):
        ops.pack_skinny_f8(q[:, :96])


def test_scales_follow_interleave_gate_up8():
    F, K = 40, 64
    w13 = _w(2 * F, K, seed=5) * torch.exp2((torch.arange(2 * F) % 7 - 3).float())[:, None].to(torch.bfloat16)
    q, s = ops.quantize_rows_fp8(w13)
    il = ops.interleave_gate_up8(w13)
    qi, si = ops.quantize_rows_fp8(il)
    assert torch.equal(si, ops.interleave_gate_up8(s[:, None])[:, 0])
    assert torch.equal(qi.view(torch.uint8), ops.interleave_gate_up8(q.view(torch.uint8)))
    assert torch.equal(ops.dequantize_rows_fp8(qi, si), ops.interleave_gate_up8(ops.dequantize_rows_fp8(q, s)))


# ------------------------------------------------------------------ the CPU reference of dec_gemm
@pytest.mark.parametrize("epi", [ops.DEC_SLAB, ops.DEC_BF16, ops.DEC_SWIGLU8])
@pytest.mark.parametrize("rn", [False, True])
def test_dec_gemm_cpu_fp8_equals_bf16_over_dequantised(epi, rn):
    N, K, M = 128, 1024, 19
    w = _w(N, K, seed=7) * torch.exp2((torch.arange(N) % 7 - 3).float())[:, None].to(torch.bfloat16)
    if epi == ops.DEC_SWIGLU8:
        w = ops.interleave_gate_up8(w)
    q, s = ops.quantize_rows_fp8(w)
    qp, wp = ops.pack_skinny_f8(q), ops.pack_skinny(ops.dequantize_rows_fp8(q, s))
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)
    a = ops.pack_activation(x)
    rownorm = ((x.float() ** 2).view(M, K // 512, 512).sum(-1), 1e-5) if rn else None
    form = next(ops.DEC_FORMS[i] for i in ops.DEC_F8_FORMS if ops.DEC_FORMS[i][0] == epi)
    for S in ((1, 2) if epi == ops.DEC_SLAB else (1,)):
        cfg = (S,) + tuple(form[1:4])
        outs = []
        for wgt, kw in ((qp, dict(wscale=s)), (wp, {})):
            if epi == ops.DEC_SLAB:
                ws = torch.full((S * M * N,), float("nan"))
                assert ops.dec_gemm(a, wgt, epi, M, workspace=ws, rownorm=rownorm, cfg=cfg, **kw) == S
                outs.append(ws)
            elif epi == ops.DEC_BF16:
                y = torch.full((M, N), float("nan"), dtype=torch.bfloat16)
                ops.dec_gemm(a, wgt, epi, M, out=y, rownorm=rownorm, cfg=cfg, **kw)
                outs.append(y)
            else:
                act = torch.full((-(-M // 16), N // 64, 64, 8), float("nan"), dtype=torch.bfloat16)
                ops.dec_gemm(a, wgt, epi, M, out=act, rownorm=rownorm, cfg=cfg, **kw)
                outs.append(ops.unpack_skinny(act)[:M])
        assert not torch.isnan(outs[0]).any()
        assert torch.equal(outs[0], outs[1]), f"epi {epi} S {S} rownorm {rn}"


def test_dec_gemm_fp8_needs_scales():
    q, _ = ops.quantize_rows_fp8(_w(16, 512))
    with pytest.raises(ValueError, match="scale"):
        ops.dec_gemm(ops.pack_activation(torch.zeros(1, 512, dtype=torch.bfloat16)), ops.pack_skinny_f8(q),
                     ops.DEC_BF16, 1, out=torch.empty(1, 16, dtype=torch.bfloat16), cfg=(1, 4, 8, 4))


# ------------------------------------------------------------------ forms
def test_f8_forms_mirror_the_native_table():
    assert tuple(ops.native().gemm_dec_f8_forms()) == tuple(ops.DEC_F8_FORMS)
    assert len(set(ops.DEC_F8_FORMS)) == len(ops.DEC_F8_FORMS)
    assert all(0 <= i < len(ops.DEC_FORMS) for i in ops.DEC_F8_FORMS)


def test_f8_forms_cover_the_llama_tables():
    for table, rows in ((ops.DEC_TABLE, (1, 64)), (ops.DEC_TABLE_M128, (65, 128))):
        for (N, K, epi), cfg in table.items():
            for r in rows:
                assert ops.dec_form_ok(epi, cfg, r, f8=True), (N, K, epi, cfg, r)
                assert ops.dec_config(N, K, epi, rows=r, f8=True) == ops.dec_config(N, K, epi, rows=r)
    cfg = ops.dec_config(57344, 8192, ops.DEC_SWIGLU8)  # Llama-3-70B gate_up at TP=1
    assert ops.dec_form_ok(ops.DEC_SWIGLU8, cfg, 64, f8=True)
    assert ops.dec_config(57344, 8192, ops.DEC_SWIGLU8, f8=True) == cfg
    # fp8 forms are dense, narrow-norm launches
    assert not ops.dec_form_ok(ops.DEC_SWIGLU8, (1, 1, 7, 8), 16, wide_norm=True, f8=True)
    assert not ops.dec_form_ok(ops.DEC_SLAB, (1, 1, 8, 8), 16, grouped=True, f8=True)
    assert ops.dec_config(4096, 14336, 0, experts=8, f8=True) is None
    # a bf16-only form is never an fp8 answer
    for N, K, epi in ((32000, 4096, 1), (6144, 4096, 0), (1024, 8192, 0)):
        for r in (1, 128):
            c = ops.dec_config(N, K, epi, rows=r, f8=True)
            assert c is None or ops.dec_form_ok(epi, c, r, f8=True)


# ------------------------------------------------------------------ engine
PROMPTS = ["pod crashloop in kube-system", "node-003 NotReady 为什么", "x" * 40]


def _engine(**kw):
    return LLMEngine(EngineConfig(model="llama-tiny", max_num_seqs=4, max_model_len=256, num_blocks=64,
                                  use_graphs=False, dtype="float32", prefix_caching=False, **kw), device="cpu")
    # (no prefix cache: these tests swap an engine's weights between runs of the same prompts)


def _greedy(eng):
    return [s.output_ids for s in eng.generate(PROMPTS, SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))]


@pytest.fixture(scope="module")
def fp8_engine():
    return _engine(decode_weights="fp8", seed=3)


def test_engine_default_is_bf16_and_fp8_is_opt_in(fp8_engine):
    assert EngineConfig().decode_weights == "bf16"
    with pytest.raises(ValueError):
        _engine(decode_weights="int4")
    m = fp8_engine.model
    st = fp8_engine.stats()
    assert st["decode_weights"] == "fp8" and st["resident_weight_bytes"] == m.resident_weight_bytes()
    assert set(st["decode_encodings"].values()) == {"fp8"}, st["decode_encodings"]
    plain = _engine(seed=3)
    assert set(plain.stats()["decode_encodings"].values()) == {"bf16"}
    assert not any(k.endswith(("_q", "_qs")) for k in plain.model.layers[0])
    assert m.resident_weight_bytes() > plain.model.resident_weight_bytes()
    assert m.num_local_params() == plain.model.num_local_params()


def test_monitor_config_passes_decode_weights_on():
    from k8s_llm_monitor_amd.monitor.app import engine_config
    from k8s_llm_monitor_amd.monitor.config import from_dict

    assert engine_config(from_dict({})).decode_weights == "bf16"
    assert engine_config(from_dict({"llm": {"decode_weights": "fp8"}})).decode_weights == "fp8"


def test_empty_init_fp8_model_quantises_what_it_is_given(fp8_engine):
    from k8s_llm_monitor_amd.models import CausalLM
    from k8s_llm_monitor_amd.parallel.state import ParallelState

    src = fp8_engine.model
    m = CausalLM(src.cfg, device="cpu", dtype=torch.float32, pstate=ParallelState(), init="empty", dec_weights="fp8")
    assert not any(k.endswith("_q") for k in m.layers[0]), "uninitialised storage is not quantised"
    m.copy_weights_from(src)
    for key in ("wqkv", "wo", "w13", "w2"):
        assert torch.equal(m.canonical(m.layers[0], key), src.canonical(src.layers[0], key)), key
        assert key + "_q" in m.layers[0]
    assert m.lm_head_q is not None


def test_engine_bf16_weights_are_the_dequantised_values(fp8_engine):
    m = fp8_engine.model
    for L in m.layers:
        for key in ("wqkv", "wo", "w13", "w2"):
            q, s = ops.unpack_skinny_f8(L[key + "_q"]), L[key + "_qs"]
            dq = ops.dequantize_rows_fp8(q, s, m.dtype)
            assert torch.equal(ops.unpack_skinny(L[key + "_d"]), dq), key
            canon = m.canonical(L, key)
            want = ops.deinterleave_gate_up8(dq) if key == "w13" else dq
            assert torch.equal(canon, want), key
            assert torch.equal(canon, canon.to(torch.bfloat16).to(canon.dtype)), "bf16-exact values"
    head = m.canonical_head()
    assert torch.equal(head, ops.dequantize_rows_fp8(ops.unpack_skinny_f8(m.lm_head_q), m.lm_head_qs, m.dtype))
    if m.cfg.tie_embeddings:
        assert torch.equal(m.embed, head), "one tensor: the embedding table takes the dequantised values too"


def test_engine_fp8_launches_fp8_weights(fp8_engine, monkeypatch):
    seen = []
    real = ops.dec_gemm

    def spy(a, wp, epi, rows, *args, **kw):
        seen.append((epi, ops.is_fp8(wp)))
        return real(a, wp, epi, rows, *args, **kw)

    monkeypatch.setattr(ops, "dec_gemm", spy)
    _greedy(fp8_engine)
    assert {e for e, f in seen if f} == {0, 1, 2}, seen[:12]


def test_engine_round_trip_bf16_engine_with_fp8_engines_weights(fp8_engine, tmp_path):
    toks = _greedy(fp8_engine)
    other = _engine(seed=9)  # other weights, bf16 decode
    assert _greedy(other) != toks
    other.model.copy_weights_from(fp8_engine.model)
    assert not any(k.endswith("_q") for k in other.model.layers[0])
    assert _greedy(other) == toks, "one model, two encodings: the same greedy tokens"
    # save -> load into an fp8 model: requantised from the dequantised values, identical logits
    save_checkpoint(fp8_engine.model, tmp_path / "ckpt")
    third = _engine(decode_weights="fp8", seed=11)
    load_checkpoint(third.model, tmp_path / "ckpt")
    for La, Lb in zip(fp8_engine.model.layers, third.model.layers):
        for key in ("wqkv", "wo", "w13", "w2"):
            assert torch.equal(third.model.canonical(Lb, key), fp8_engine.model.canonical(La, key)), key
            assert torch.equal(ops.dequantize_rows_fp8(ops.unpack_skinny_f8(Lb[key + "_q"]), Lb[key + "_qs"]),
                               ops.dequantize_rows_fp8(ops.unpack_skinny_f8(La[key + "_q"]), La[key + "_qs"])), key
    assert _greedy(third) == toks
    # copy_weights_from INTO an fp8 model rebuilds its codes from the new weights
    src = _engine(seed=9)
    third.model.copy_weights_from(src.model)
    L = third.model.layers[0]
    assert torch.equal(ops.unpack_skinny(L["wo_d"]),
                       ops.dequantize_rows_fp8(ops.unpack_skinny_f8(L["wo_q"]), L["wo_qs"], third.model.dtype))
    assert not torch.equal(third.model.canonical(L, "wo"), fp8_engine.model.canonical(fp8_engine.model.layers[0], "wo"))
