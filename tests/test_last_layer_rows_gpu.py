"""CausalLM.LAST_LAYER_ROWS: the last layer of a dense TP = 1 prefill runs o, gate_up and down on the
rows of ``meta.logits_idx`` only.  Every GEMM of that tail treats its rows alone, so with the constant
on and off the logits AND the KV caches must be bitwise equal: a prefill of two prompts (5 + 9 tokens)
with one logit row each, a chunk that ends inside both prompts (no logit rows: the tail is skipped),
and - the headline's path - a step of at least ops.TILE_MIN_M rows, which takes the fused-norm layer
(_prefill_fused_norm).  The short cases run on the CPU path as well."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.models import AttnMeta, CausalLM
from k8s_llm_monitor_amd.models.config import get_config

NB = 80  # 16-token cache blocks: 1280 slots


def _step(model, lens, rows, device):
    """One prefill step over prompts of ``lens`` tokens writing a fresh paged cache; ``rows``: logits_idx.
    Returns (logits, k cache, v cache)."""
    c = model.cfg
    T = sum(lens)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    ids = torch.tensor([(7 * i + 3) % c.vocab_size for i in range(T)], dtype=torch.int32, device=device)
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).to(device)
    first = [16 * sum((m + 15) // 16 for m in lens[:j]) for j in range(len(lens))]  # each prompt in blocks of its own
    slots = torch.cat([torch.arange(n, dtype=torch.int32) + f for n, f in zip(lens, first)])
    assert int(slots.max()) < NB * 16
    k, v = ops.kv_cache_alloc(c.n_layers, NB, c.n_kv_heads, c.head_dim, model.dtype, device)
    qs, st = ops.prefill_qblocks(cu)
    meta = AttnMeta(is_prefill=True, positions=pos, slot_mapping=slots.to(device),
                    cu_seqlens=torch.tensor(cu, dtype=torch.int32, device=device),
                    qb_seq=torch.tensor(qs, dtype=torch.int32, device=device),
                    qb_start=torch.tensor(st, dtype=torch.int32, device=device),
                    logits_idx=torch.tensor(rows, dtype=torch.int64, device=device))
    with torch.no_grad():
        lg = model.forward(ids, meta, [(k[i], v[i]) for i in range(c.n_layers)])
    return lg, k, v


def _on_off(model, lens, rows, device, seen=None):
    out = []
    for on in (True, False):
        model.LAST_LAYER_ROWS = on
        try:
            calls, real_t, real_r = [], ops.gemm_tile, ops.gemm_tile_resid
            ops.gemm_tile = lambda x, *a, **kw: (calls.append(x.shape[0]), real_t(x, *a, **kw))[1]
            ops.gemm_tile_resid = lambda x, *a, **kw: (calls.append(x.shape[0]), real_r(x, *a, **kw))[1]
            try:
                out.append(_step(model, lens, rows, device))
            finally:
                ops.gemm_tile, ops.gemm_tile_resid = real_t, real_r
            if seen is not None:
                seen[on] = calls
        finally:
            del model.LAST_LAYER_ROWS
    (la, ka, va), (lb, kb, vb) = out
    assert la.shape == (len(rows), model.cfg.vocab_size) and la.dtype == lb.dtype
    assert torch.isfinite(la.float()).all()
    assert torch.equal(la, lb), "logits differ between LAST_LAYER_ROWS on and off"
    assert torch.equal(ka, kb) and torch.equal(va, vb), "KV caches differ"
    assert ka.float().abs().sum() > 0 and va.float().abs().sum() > 0
    return la


CASES = {"prompts_5_9": ((5, 9), [4, 13]), "chunk_no_logit_rows": ((4, 6), [])}


@pytest.mark.parametrize("layout", [True, "force"], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("case", CASES)
def test_cpu_path(case, layout):
    CausalLM.ONE_LAYOUT = layout
    try:
        model = CausalLM(get_config("llama-tiny-d128"), device="cpu", seed=3)
    finally:
        CausalLM.ONE_LAYOUT = True
    assert (model.layers[0]["wo"].dim() == 4) == (layout == "force")
    _on_off(model, *CASES[case], "cpu")


@pytest.fixture(scope="module")
def gpu_model():
    return CausalLM(get_config("llama-tiny-d128"), device="cuda", seed=3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_short_prefill(gpu_model, case):
    """Below ops.TILE_MIN_M rows: forward's layer loop, every projection on the tile kernel over the
    packed weights."""
    seen = {}
    lens, rows = CASES[case]
    _on_off(gpu_model, lens, rows, "cuda", seen)
    T = sum(lens)
    assert seen[False] and all(m == T for m in seen[False])
    # on: the two layers' qkv and layer 0's three others see every row, the last layer's tail the logit rows
    assert sorted(seen[True]) == sorted([T] * 5 + [len(rows)] * (3 if rows else 0))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [[699, 1099], [0, 511, 699, 700, 1099], []], ids=["last_tokens", "five_rows", "none"])
def test_gpu_fused_norm_prefill(gpu_model, rows):
    """700 + 400 tokens: the fused-norm layer (the residual epilogue and the row scale)."""
    lens = (700, 400)
    assert gpu_model._fused_norm_ok(torch.empty(sum(lens), gpu_model.cfg.d_model, device="cuda", dtype=torch.bfloat16))
    seen = {}
    _on_off(gpu_model, lens, rows, "cuda", seen)
    assert sorted(seen[True]) == sorted([1100] * 5 + [len(rows)] * (3 if rows else 0))
    assert seen[False] == [1100] * 8
