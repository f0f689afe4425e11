"""A 128-row decode batch through the engine at Llama-3-8B dimensions (2 layers): the 128-row
hipGraph bucket runs every projection and the LM head on gemm_decode.hip's 5..8 m-tile kernels.

Ten sequences - both ends of m-tiles 5 to 8 and the old 64-row boundary - are checked against the
fp32 CPU reference holding the same weights, by the rule of
tests/test_real_shape_gpu.py::test_gpu_real_shape_decode_batch64_matches_fp32_reference: GPU
prefill logits within 0.03 x scale of fp32, every greedy token within 2 x err of the fp32 argmax.
The other 118 are checked against the GPU's own teacher-forced prefill logits ``lg`` (no CPU
forward): each decoded token's ``lg`` value within 4 x E of the row's ``lg`` maximum, E the largest
err of the ten (2 E for decode against fp32, plus E on each side for ``lg`` against fp32).
A second run of 100 prompts decodes in the 112-row bucket with 12 padding rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N_NEW = 6
CHECKED = [0, 63, 64, 79, 80, 95, 96, 111, 112, 127]


def _fp32_reference(gpu_model):  # as tests/test_real_shape_gpu.py
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
    """Teacher-forced prefill forward of one sequence; logits of ``rows`` as fp32 on the CPU."""
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


@pytest.fixture(scope="module")
def run():
    from k8s_llm_monitor_amd import ops
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams

    torch.set_num_threads(16)
    eng = LLMEngine(EngineConfig(model="llama-3-8b", model_overrides={"n_layers": 2}, max_num_seqs=128,
                                 max_model_len=1024, kv_cache_gb=4.0, seed=5), device="cuda")
    # count the rows ops.dec_gemm is launched with while the decode graphs are captured: what a
    # bucket's graph replays is what its capture launched
    seen, real = [], ops.dec_gemm

    def spy(a, wp, epi, rows, *args, **kw):
        seen.append((epi, rows))
        return real(a, wp, epi, rows, *args, **kw)

    ops.dec_gemm = spy
    try:
        eng.warmup()
    finally:
        ops.dec_gemm = real
    sp = SamplingParams(max_tokens=N_NEW, temperature=0.0, ignore_eos=True)
    seqs128 = eng.generate(_prompts(128, "a"), sp)
    steps128 = [n for (n, _, _) in eng.step_samples]
    eng.step_samples.clear()
    seqs100 = eng.generate(_prompts(100, "b"), sp)
    steps100 = [n for (n, _, _) in eng.step_samples]
    torch.cuda.synchronize()
    out = {"eng": eng, "seen": seen, "seqs128": seqs128, "seqs100": seqs100, "steps128": steps128,
           "steps100": steps100, "ref": _fp32_reference(eng.model)}
    yield out
    out.clear()
    del eng
    torch.cuda.empty_cache()


def _rows(s):
    p = len(s.prompt_ids)
    return s.prompt_ids + s.output_ids, list(range(p - 1, p - 1 + N_NEW))


def _check_fp32(run, seqs, which):
    """The batch-64 test's rule on sequences ``which``; returns the largest err."""
    E = 0.0
    for i in which:
        s = seqs[i]
        assert len(s.output_ids) == N_NEW
        ids, rows = _rows(s)
        lr = _logits(run["ref"], ids, rows, "cpu")
        lg = _logits(run["eng"].model, ids, rows, "cuda")
        scale = float(lr.abs().max())
        err = float((lg - lr).abs().max())
        print(f"seq {i}: prefill logits max-abs err {err:.4f} scale {scale:.3f}")
        assert err < 0.03 * scale, f"row {i}: prefill logits max-abs err {err:.4f} vs scale {scale:.3f}"
        for t in range(N_NEW):
            top, got = float(lr[t].max()), float(lr[t, s.output_ids[t]])
            assert top - got <= 2 * err + 1e-6, (
                f"row {i} step {t}: token {s.output_ids[t]} logit {got:.4f} vs max {top:.4f} (bf16 err {err:.4f})")
        E = max(E, err)
    return E


def _check_lg(run, seqs, which, E):
    worst = 0.0
    for i in which:
        s = seqs[i]
        assert len(s.output_ids) == N_NEW
        ids, rows = _rows(s)
        lg = _logits(run["eng"].model, ids, rows, "cuda")
        for t in range(N_NEW):
            top, got = float(lg[t].max()), float(lg[t, s.output_ids[t]])
            worst = max(worst, top - got)
            assert top - got <= 4 * E + 1e-6, (
                f"row {i} step {t}: token {s.output_ids[t]} GPU prefill logit {got:.4f} vs its max {top:.4f} (E {E:.4f})")
    print(f"{len(which)} sequences against GPU prefill logits: worst gap {worst:.4f}, bound {4 * E:.4f}")


def test_128_row_bucket_runs_dec_gemm(run):
    st = run["eng"].stats()
    assert 128 in st["graph_buckets"] and {80, 96, 112} <= set(st["graph_buckets"])
    assert run["eng"].model.dec_rows_max() == 128
    wide = {(epi, r) for epi, r in run["seen"] if r > 64}
    for epi in (0, 1, 2):  # slabs, the LM head and the SwiGLU epilogue, all in the 128-row capture
        assert (epi, 128) in wide, f"epilogue {epi} not launched with 128 rows: {sorted(wide)}"
    assert {r for _, r in wide} >= {80, 96, 112, 128}
    assert 128 in run["steps128"], "a decode step held all 128 sequences"


def test_128_sequences_match_fp32_and_prefill(run):
    seqs = run["seqs128"]
    assert len(seqs) == 128
    E = _check_fp32(run, seqs, CHECKED)
    _check_lg(run, seqs, [i for i in range(128) if i not in CHECKED], E)


def test_100_sequences_in_the_112_row_bucket(run):
    seqs = run["seqs100"]
    assert len(seqs) == 100 and 100 in run["steps100"]
    assert run["eng"].runner.bucket_for(100) == 112
    chk = [0, 64, 96, 99]
    E = _check_fp32(run, seqs, chk)
    _check_lg(run, seqs, [i for i in range(100) if i not in chk], E)
