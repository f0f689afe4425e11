"""A MoE engine (mixtral-tiny-d128, graphs on, up to 64 rows per step) decoding its expert stacks
from fp8 and from mxfp4 codes: tests/test_fp8_engine_gpu.py for the grouped launches.

The decode graphs must have captured quantised grouped launches (ops.dec_gemm_grouped_q) of the
SwiGLU and the slab epilogue in a bucket of at most 16 rows and in the 64-row bucket.  Batches of 3
and of 64 prompts must come out token for token as from a bf16-decoding engine given the same
weights (the quantised launches are bit-identical to the bf16 ones over the dequantised stacks), and
are checked against the fp32 CPU model given those weights through copy_weights_from - so the
reference computes with exactly the weights the kernels stream: GPU prefill logits within 0.03 x
scale, every greedy token within 2 x err of the fp32 argmax."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N_NEW = 6
CHECKED_64 = [0, 31, 63]


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


def _prompts(n, tag):
    return [f"{tag} node-{i:03d} CPU={30 + i % 60}% pod payments-{i} restarts={i % 7} 为什么我的pod频繁重启？" for i in range(n)]


def _cfg(seed=5, **kw):
    from k8s_llm_monitor_amd.engine import EngineConfig

    return EngineConfig(model="mixtral-tiny-d128", max_num_seqs=64, max_model_len=1024, kv_cache_gb=1.0, seed=seed,
                        prefix_caching=False, **kw)


@pytest.fixture(scope="module", params=("fp8", "mxfp4"))
def run(request):
    from k8s_llm_monitor_amd import ops
    from k8s_llm_monitor_amd.engine import LLMEngine, SamplingParams

    enc = request.param
    torch.set_num_threads(16)
    eng = LLMEngine(_cfg(decode_weights=enc), device="cuda")
    seen, real = [], ops.dec_gemm_grouped_q

    def spy(a, wq, wqs, epi, rows, **kw):  # what a bucket's graph replays is what its capture launched
        seen.append((epi, rows, "mxfp4" if ops.is_mxfp4(wq) else "fp8" if ops.is_fp8(wq) else "?"))
        return real(a, wq, wqs, epi, rows, **kw)

    ops.dec_gemm_grouped_q = spy
    try:
        eng.warmup()
    finally:
        ops.dec_gemm_grouped_q = real
    sp = SamplingParams(max_tokens=N_NEW, temperature=0.0, ignore_eos=True)
    seqs3 = eng.generate(_prompts(3, "c"), sp)
    seqs64 = eng.generate(_prompts(64, "a"), sp)
    torch.cuda.synchronize()
    out = {"enc": enc, "eng": eng, "seen": seen, "seqs3": seqs3, "seqs64": seqs64, "ref": _fp32_reference(eng.model),
           "sp": sp}
    yield out
    out.clear()
    del eng
    torch.cuda.empty_cache()


def test_quantised_grouped_launches_in_small_and_64_row_buckets(run):
    from k8s_llm_monitor_amd import ops

    eng, enc = run["eng"], run["enc"]
    st = eng.stats()
    assert st["decode_weights"] == enc
    assert st["decode_encodings"]["w13"] == st["decode_encodings"]["w2"] == enc, st["decode_encodings"]
    assert 64 in st["graph_buckets"] and eng.runner.graphs
    assert {e for _, _, e in run["seen"]} == {enc}
    got = {(epi, r) for epi, r, _ in run["seen"]}
    small = {epi for epi, r in got if r <= 16}
    for epi in (ops.DEC_SWIGLU8, ops.DEC_SLAB):
        assert epi in small, f"epilogue {epi}: no {enc} grouped launch at <= 16 rows: {sorted(got)}"
        assert (epi, 64) in got, f"epilogue {epi}: no {enc} grouped launch at 64 rows: {sorted(got)}"
    # resident weights: the expert stacks' codes and scales are counted, once
    m = eng.model
    E = m.cfg.n_experts
    stack_q = 0
    for L in m.layers:
        for key in ("w13", "w2"):
            q, s, w = L[key + "_q"], L[key + "_qs"], L[key + "_dg"]
            assert q.dim() == 5 and q.shape[0] == E and L[key] is w
            n = w.numel()
            assert q.numel() * q.element_size() == (n if enc == "fp8" else n // 2)
            assert s.numel() * s.element_size() == (4 * n // w.shape[2] // 32 if enc == "fp8" else n // 32)
            stack_q += q.numel() * q.element_size() + s.numel() * s.element_size()
    all_q = sum(v.numel() * v.element_size() for L in m.layers for k, v in L.items() if k.endswith(("_q", "_qs")))
    all_q += sum(t.numel() * t.element_size() for t in (m.lm_head_q, m.lm_head_qs))
    assert all_q > stack_q > all_q // 2, "the expert stacks are most of what is quantised"
    assert st["resident_weight_bytes"] == m.resident_weight_bytes()


def _check_fp32(run, seqs, which):
    for i in which:
        s = seqs[i]
        assert len(s.output_ids) == N_NEW
        p = len(s.prompt_ids)
        ids, rows = s.prompt_ids + s.output_ids, list(range(p - 1, p - 1 + N_NEW))
        lr = _logits(run["ref"], ids, rows, "cpu")
        lg = _logits(run["eng"].model, ids, rows, "cuda")
        scale = float(lr.abs().max())
        err = float((lg - lr).abs().max())
        print(f"{run['enc']} seq {i}: prefill logits max-abs err {err:.4f} scale {scale:.3f}")
        assert err < 0.03 * scale, f"row {i}: prefill logits max-abs err {err:.4f} vs scale {scale:.3f}"
        for t in range(N_NEW):
            top, got = float(lr[t].max()), float(lr[t, s.output_ids[t]])
            assert top - got <= 2 * err + 1e-6, (
                f"row {i} step {t}: token {s.output_ids[t]} logit {got:.4f} vs max {top:.4f} (bf16 err {err:.4f})")


def test_batch_of_3_matches_fp32_over_the_dequantised_weights(run):
    assert len(run["seqs3"]) == 3
    _check_fp32(run, run["seqs3"], range(3))


def test_batch_of_64_matches_fp32_over_the_dequantised_weights(run):
    assert len(run["seqs64"]) == 64 and all(len(s.output_ids) == N_NEW for s in run["seqs64"])
    _check_fp32(run, run["seqs64"], CHECKED_64)


def test_bf16_decoding_engine_with_the_same_weights_emits_identical_tokens(run):
    from k8s_llm_monitor_amd.engine import LLMEngine

    eng = LLMEngine(_cfg(seed=6), device="cuda")
    assert set(eng.stats()["decode_encodings"].values()) == {"bf16"}
    eng.model.copy_weights_from(run["eng"].model)
    assert "w13_q" not in eng.model.layers[0]
    q_bytes = sum(v.numel() * v.element_size() for L in run["eng"].model.layers for k, v in L.items()
                  if k.endswith(("_q", "_qs")))
    q_bytes += sum(t.numel() * t.element_size() for t in (run["eng"].model.lm_head_q, run["eng"].model.lm_head_qs))
    assert run["eng"].stats()["resident_weight_bytes"] == eng.stats()["resident_weight_bytes"] + q_bytes
    eng.warmup()
    for n, tag, key in ((3, "c", "seqs3"), (64, "a", "seqs64")):
        seqs = eng.generate(_prompts(n, tag), run["sp"])
        torch.cuda.synchronize()
        assert [s.output_ids for s in seqs] == [s.output_ids for s in run[key]], f"batch of {n}"
    del eng
    torch.cuda.empty_cache()
