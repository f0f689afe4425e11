"""prefill_weights="mxfp4" end to end at Llama-3-8B dimensions (2 layers): an engine whose dense
projections and LM head are resident as mxfp4 codes and block scales ONLY against an engine with
decode_weights="mxfp4" alone (codes beside the bf16 copy), same seed, so both hold the same values.

Every prefill projection of the codes-only engine must launch the tile GEMM over an mxfp4 W, with
all six (epilogue, row scale) kinds seen: RoPE and SwiGLU8 with and without the row scale (with:
the fused-norm layer, from ops.TILE_MIN_M rows), the residual epilogue and the plain one (a short
prompt).  Greedy tokens and prefill logits must be IDENTICAL between the two engines (the mxfp4-W
tile GEMM is bit-identical to the bf16 one and decode runs the same launches), and sequence 0
passes the fp32 rule of tests/test_fp8_engine_gpu.py against the fp32 CPU model given the
dequantised weights through copy_weights_from.

The engines run with max_model_len 1024, which admits prompts below 1024 tokens only; the prompt
of >= 1024 tokens that takes the fused-norm layer goes through the models' prefill forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N_NEW = 6
LONG = 1100  # >= ops.TILE_MIN_M rows in one prefill: the RMSNorms move into the GEMM epilogues


def _fp32_reference(gpu_model):  # as tests/test_fp8_engine_gpu.py
    from k8s_llm_monitor_amd.models import CausalLM
    from k8s_llm_monitor_amd.parallel.state import ParallelState

    CausalLM.SKINNY_DECODE = False  # the reference runs the plain row-major path only
    try:
        ref = CausalLM(gpu_model.cfg, device="cpu", dtype=torch.float32, pstate=ParallelState(), init="empty")
    finally:
        CausalLM.SKINNY_DECODE = True
    ref.copy_weights_from(gpu_model)
    return ref


def _logits(model, ids, rows, device):
    from k8s_llm_monitor_amd.models import AttnMeta

    n = len(ids)
    t = torch.tensor(ids, dtype=torch.int32, device=device)
    meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32, device=device),
                    slot_mapping=torch.full((n,), -1, dtype=torch.int32, device=device),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32, device=device),
                    logits_idx=torch.tensor(rows, device=device))
    return model.forward(t, meta, None).float().cpu()


def _prompts(n):
    return [f"c node-{i:03d} CPU={30 + i % 60}% pod payments-{i} restarts={i % 7} 为什么我的pod频繁重启？" for i in range(n)]


def _engine(**kw):
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine

    return LLMEngine(EngineConfig(model="llama-3-8b", model_overrides={"n_layers": 2}, max_num_seqs=8,
                                  max_model_len=1024, kv_cache_gb=1.0, seed=5, prefix_caching=False,
                                  decode_weights="mxfp4", **kw), device="cuda")


@pytest.fixture(scope="module")
def run():
    from k8s_llm_monitor_amd import ops
    from k8s_llm_monitor_amd.engine import SamplingParams

    torch.set_num_threads(16)
    sp = SamplingParams(max_tokens=N_NEW, temperature=0.0, ignore_eos=True)
    long_ids = [(7 * i + 3) % 32000 for i in range(LONG)]
    long_rows = [0, 511, LONG - 1]
    both = _engine()
    both.warmup()
    toks_both = [s.output_ids for s in both.generate(_prompts(3), sp)]
    long_both = _logits(both.model, long_ids, long_rows, "cuda")
    torch.cuda.synchronize()
    bytes_both = both.stats()["resident_weight_bytes"]
    # the bf16 copies that go: a code byte holds two elements, a bf16 element is two bytes
    released = sum(4 * L[k + "_q"].numel() for L in both.model.layers for k in ("wqkv", "wo", "w13", "w2"))
    released += 4 * both.model.lm_head_q.numel()
    enc_both = both.stats()["prefill_encodings"]
    del both
    torch.cuda.empty_cache()

    only = _engine(prefill_weights="mxfp4")
    seen, real_t, real_r = [], ops.gemm_tile, ops.gemm_tile_resid

    def spy_t(x, w, offsets=None, swiglu=False, *a, **kw):
        epi = "rope" if kw.get("rope") is not None else "swiglu8" if swiglu == 8 else "swiglu" if swiglu else "plain"
        seen.append((epi, kw.get("rowscale") is not None, ops.is_mxfp4(w), x.shape[0]))
        return real_t(x, w, offsets, swiglu, *a, **kw)

    def spy_r(x, w, *a, **kw):
        seen.append(("resid", False, ops.is_mxfp4(w), x.shape[0]))
        return real_r(x, w, *a, **kw)

    ops.gemm_tile, ops.gemm_tile_resid = spy_t, spy_r
    try:
        only.warmup()
        seqs = only.generate(_prompts(3), sp)
        long_only = _logits(only.model, long_ids, long_rows, "cuda")
    finally:
        ops.gemm_tile, ops.gemm_tile_resid = real_t, real_r
    torch.cuda.synchronize()
    out = {"only": only, "seen": seen, "seqs": seqs, "toks_both": toks_both, "long": (long_both, long_only),
           "bytes_both": bytes_both, "released": released, "enc_both": enc_both}
    yield out
    out.clear()
    del only
    torch.cuda.empty_cache()


def test_every_prefill_projection_launched_an_mxfp4_weight(run):
    seen = run["seen"]
    assert seen and all(f4 for _, _, f4, _ in seen), [s for s in seen if not s[2]][:8]
    kinds = {(epi, rs) for epi, rs, _, _ in seen}
    for want in (("rope", False), ("rope", True), ("resid", False), ("swiglu8", True), ("swiglu8", False),
                 ("plain", False)):
        assert want in kinds, f"{want} never launched: {sorted(kinds)}"
    from k8s_llm_monitor_amd import ops
    assert any(epi == "plain" and m < ops.TILE_MIN_M for epi, _, _, m in seen), "a short prompt's plain projections"
    assert any(epi == "resid" and m >= ops.TILE_MIN_M for epi, _, _, m in seen)


def test_stats_report_codes_only_and_the_released_bytes(run):
    st = run["only"].stats()
    assert st["decode_weights"] == "mxfp4" and st["prefill_weights"] == "mxfp4"
    assert set(st["prefill_encodings"].values()) == {"mxfp4"}, st["prefill_encodings"]
    assert set(run["enc_both"].values()) == {"bf16"}
    assert set(st["decode_encodings"].values()) == {"mxfp4"}
    assert st["resident_weight_bytes"] == run["only"].model.resident_weight_bytes()
    assert run["bytes_both"] - st["resident_weight_bytes"] == run["released"] > 0
    m = run["only"].model
    from k8s_llm_monitor_amd import ops
    assert all(ops.is_mxfp4(L[k]) and L[k] is L[k + "_q"] and k + "_d" not in L
               for L in m.layers for k in ("wqkv", "wo", "w13", "w2"))
    assert m.lm_head_d is None and ops.is_mxfp4(m.lm_head) and m.dec_rows_max() == 128


def test_tokens_and_prefill_logits_identical_to_the_two_copy_engine(run):
    assert all(len(s.output_ids) == N_NEW for s in run["seqs"])
    assert [s.output_ids for s in run["seqs"]] == run["toks_both"]
    a, b = run["long"]
    assert torch.isfinite(b).all() and torch.equal(a, b), "prefill logits of the 1100-token prompt"


def test_sequence_0_matches_fp32_over_the_dequantised_weights(run):
    ref = _fp32_reference(run["only"].model)
    s = run["seqs"][0]
    p = len(s.prompt_ids)
    ids, rows = s.prompt_ids + s.output_ids, list(range(p - 1, p - 1 + N_NEW))
    lr = _logits(ref, ids, rows, "cpu")
    lg = _logits(run["only"].model, ids, rows, "cuda")
    scale = float(lr.abs().max())
    err = float((lg - lr).abs().max())
    print(f"seq 0: prefill logits max-abs err {err:.4f} scale {scale:.3f}")
    assert err < 0.03 * scale, f"prefill logits max-abs err {err:.4f} vs scale {scale:.3f}"
    for t in range(N_NEW):
        top, got = float(lr[t].max()), float(lr[t, s.output_ids[t]])
        assert top - got <= 2 * err + 1e-6, (
            f"step {t}: token {s.output_ids[t]} logit {got:.4f} vs max {top:.4f} (bf16 err {err:.4f})")
