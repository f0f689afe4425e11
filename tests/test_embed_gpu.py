"""Embedding requests on the GPU: pool.hip against the fp64 reference at every width, row count,
input type and alignment it distinguishes, and ``engine.embed`` (graphs and pipelining on) against
an fp32 CPU forward of the same weights through every scheduling path."""
import numpy as np
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.models import AttnMeta, CausalLM
from k8s_llm_monitor_amd.models.reference import fp32_hidden, fp32_logits
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.5
ROWS = (1, 3, 64, 130)


# ---------------------------------------------------------------- 1. the kernel

def _dims(mode, R, d):
    if mode == "full":
        return [d] * R
    if mode == "8":
        return [8] * R
    if mode == "half":
        return [d // 2] * R
    # a different value per row: both sides of every 8-column group and of the 2048-column stride of
    # the workgroup, one column, all of them - and rows that are no embedding rows (0, -1)
    pool = [d, 1, 7, 9, d // 2 + 3, 0, d - 1, -1, 16, min(d, 2049), d // 2, min(d, 2047)]
    return [pool[r % len(pool)] for r in range(R)]


# pad 4: with d = 132 / 516 the bf16 rows are 16-byte aligned too (pad 0 aligns only their fp32 rows)
@pytest.mark.parametrize("pad", [0, 8, 4, 3], ids=["dense", "strided", "strided-4", "strided-unaligned"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [64, 128, 132, 516, 520, 4096, 5120])  # 132, 516: a vector body and a scalar tail
def test_pool_l2_kernel(d, dtype, pad):
    """|e - ref| <= (dim / 2 + 8) * 2^-24 * |ref| elementwise: the inputs (bf16 values, also in the
    fp32 case) and their squares are exact in fp32; a sum of ``dim`` positive terms is within
    (dim - 1) * 2^-24 relative whatever its order, the inverse square root halves that, and 8 units
    cover the rsqrt instruction and the final multiply."""
    g = torch.Generator().manual_seed(d + pad)
    for R in ROWS:
        wide = (torch.randn(R, d + pad, generator=g) * 3).bfloat16()
        if R > 1:
            wide[R // 2] = 0  # one all-zero row
        x_cpu = wide[:, :d]
        xw = wide.to(dtype).to(DEV)
        x = xw[:, :d]
        assert x.stride(0) == d + pad
        for mode in ("full", "8", "half", "rows"):
            dim = _dims(mode, R, d)
            buf = torch.full((R + 1, d), SENTINEL, dtype=torch.float32, device=DEV)  # a sentinel row after the output
            out = ops.pool_l2(x, torch.tensor(dim, dtype=torch.int32, device=DEV), out=buf[:R])
            assert out.data_ptr() == buf.data_ptr()
            again = ops.pool_l2(x, dim)  # host dims; a fresh output
            torch.cuda.synchronize()
            got = buf.cpu()
            want = ref.pool_l2(x_cpu.double(), dim, torch.full((R, d), SENTINEL, dtype=torch.float32))
            want64 = torch.zeros(R, d, dtype=torch.float64)
            for r, n in enumerate(dim):
                if n > 0 and float(x_cpu[r, :n].double().norm()) > 0:
                    want64[r, :n] = x_cpu[r, :n].double() / x_cpu[r, :n].double().norm()
            assert torch.all(got[R] == SENTINEL), "the row after the output is intact"
            for r, n in enumerate(dim):
                if n <= 0:
                    assert torch.all(got[r] == SENTINEL), (R, mode, r, "a row that is no embedding row is untouched")
                    assert torch.all(again[r] == 0)
                    continue
                assert torch.all(got[r, n:] == 0), (R, mode, r)
                tol = (n / 2 + 8) * 2.0 ** -24 * want64[r, :n].abs()
                err = (got[r, :n].double() - want64[r, :n]).abs()
                assert torch.all(err <= tol), (R, mode, r, n, float((err / tol.clamp_min(1e-300)).max()))
                assert torch.equal(again[r].cpu(), got[r]), "two launches give the same bits"
            assert not torch.isnan(got).any()
            assert torch.allclose(want[:R], got[:R], rtol=1e-5, atol=0), "and the fp32 reference agrees"


def test_pool_l2_refusals_on_the_gpu():
    x = torch.randn(3, 64, device=DEV).bfloat16()
    ok = torch.tensor([64, 64, 64], dtype=torch.int32, device=DEV)
    for bad in (lambda: ops.pool_l2(x, [64, 65, 1]), lambda: ops.pool_l2(x.view(3, 8, 8), ok),
                lambda: ops.pool_l2(x, ok, out=torch.zeros(3, 64, dtype=torch.bfloat16, device=DEV)),
                lambda: ops.pool_l2(x, ok, out=torch.zeros(4, 64, device=DEV)),
                lambda: ops.pool_l2(x, ok, out=torch.zeros(3, 128, device=DEV)[:, :64]),
                lambda: ops.pool_l2(x, ok.long()), lambda: ops.pool_l2(x, ok[:2]),
                lambda: ops.pool_l2(x.half(), ok)):
        with pytest.raises(ValueError, match="pool_l2"):
            bad()
    assert ops.pool_l2(x[:0], ok[:0]).shape == (0, 64)


# ---------------------------------------------------------------- 2. engine values

MODELS = ["llama-tiny-d128", "qwen3-tiny-d128"]
B = 8


def _ids(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 1000, (n,), generator=g).tolist()


PROMPT = _ids(40, 0)
OTHERS = [_ids(n, 100 + n) for n in (1, 2, 15, 16, 17, 100, 300)]


def _engine(name, **kw):
    cfg = dict(model=name, max_num_seqs=B, max_model_len=1024, num_blocks=256, seed=0)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device=DEV)


@pytest.fixture(scope="module", params=MODELS)
def served(request):
    """One warmed-up engine per model (graphs captured, pipelining on) and its fp32 CPU references."""
    eng = _engine(request.param)
    eng.warmup()
    cache = {}

    def want(ids):
        key = tuple(ids)
        if key not in cache:
            h = fp32_hidden(eng.model, torch.tensor(ids), device="cpu")
            cache[key] = ref.pool_l2(h, [h.shape[1]])[0].numpy()
        return cache[key]

    return eng, want


def _close(e, want):
    """smoke()'s bf16-against-fp32 bound: 3 % of the scale."""
    assert e is not None and e.dtype == np.float32 and e.shape == want.shape
    err, scale = float(np.abs(e - want).max()), float(np.abs(want).max())
    assert err <= 0.03 * scale, f"max |e - e_ref| = {err:.5f} > 3 % of {scale:.5f}"


def test_gpu_engine_alone_among_others_and_cached(served):
    eng, want = served
    assert eng.cfg.use_graphs and eng.cfg.pipeline and eng.runner.graphs
    (e,) = eng.embed([PROMPT])
    _close(e, want(PROMPT))
    ctx0 = eng.runner.n_steps["prefill_context_tokens"]
    (again,) = eng.embed([PROMPT])  # a prefix-cache hit: two blocks attended, eight tokens computed
    assert eng.runner.n_steps["prefill_context_tokens"] == ctx0 + 32
    _close(again, want(PROMPT))
    vecs = eng.embed(OTHERS[:3] + [PROMPT] + OTHERS[3:])
    for ids, v in zip(OTHERS[:3] + [PROMPT] + OTHERS[3:], vecs):
        _close(v, want(ids))
    (cut,) = eng.embed([PROMPT], dim=8)
    w8 = want(PROMPT)[:8] / np.linalg.norm(want(PROMPT)[:8])
    _close(cut, w8.astype(np.float32))


def test_gpu_engine_three_chunks(served):
    big, want = served
    eng = _engine(big.model_cfg.name, max_prefill_tokens=16)
    (e,) = eng.embed([PROMPT])
    assert eng.counters["prefill_steps"] == 3
    _close(e, want(PROMPT))
    # the token budget, not the batch, bounds these steps: each is enqueued behind the one before it
    for ids, v in zip((OTHERS[5], PROMPT, OTHERS[4]), eng.embed([OTHERS[5], PROMPT, OTHERS[4]])):
        _close(v, want(ids))


def test_gpu_engine_pipelined_prefill_steps_reuse_both_buffers(served):
    eng, want = served
    prompts = [_ids(5 + 3 * i, 500 + i) for i in range(3 * B)]
    p0 = eng.counters["prefill_steps"]
    seqs = [eng.add_request(p, embed=True) for p in prompts]
    while eng.has_work():
        eng.step()
    assert eng.counters["prefill_steps"] - p0 >= 3, "more sequences than the batch holds: several prefill steps"
    assert all(b is not None for b in eng.runner._pf_emb), "both pinned buffers were used"
    for p, s in zip(prompts, seqs):
        assert s.finish_reason == "embed"
        _close(s.embedding, want(p))


# ---------------------------------------------------------------- 3. interleaved with generation, 4. the head spy

class HeadSpy:
    def __init__(self, monkeypatch):
        self.rows = []
        orig = CausalLM._logits

        def spy(model, x, rows=None):
            self.rows.append(int(x.shape[0]) if rows is None else int(rows))
            return orig(model, x, rows)

        monkeypatch.setattr(CausalLM, "_logits", spy)


def _smoke_criterion(eng, s, n_chk=4):
    """smoke()'s check of a generated sequence: the GPU prefill logits of prompt + first tokens within
    3 % of the fp32 CPU logits' scale, every token the fp32 argmax or a near-tie within twice that error."""
    full = list(s.prompt_ids) + list(s.output_ids[:n_chk])
    T, n, dev = len(s.prompt_ids), len(s.prompt_ids) + n_chk, eng.device
    rows = list(range(T - 1, T - 1 + n_chk))
    meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32, device=dev),
                    slot_mapping=torch.full((n,), -1, dtype=torch.int32, device=dev),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32, device=dev),
                    logits_idx=torch.tensor(rows, device=dev))
    with torch.no_grad():
        lg = eng.model.forward(torch.tensor(full, dtype=torch.int32, device=dev), meta, None).float().cpu()
    lr = fp32_logits(eng.model, torch.tensor(full), rows, device="cpu")
    scale, err = float(lr.abs().max()), float((lg - lr).abs().max())
    assert err < 0.03 * scale
    for t in range(n_chk):
        top, got = float(lr[t].max()), float(lr[t, s.output_ids[t]])
        assert top - got <= 2 * err + 1e-6, (t, s.output_ids[t], top, got, err)


def test_gpu_interleaved_with_generation(served, monkeypatch):
    eng, want = served
    r = eng.runner
    captures = []
    orig = r.capture_graphs
    monkeypatch.setattr(r, "capture_graphs", lambda *a, **k: captures.append(a) or orig(*a, **k))
    buckets, graphs = eng.stats()["graph_buckets"], {b: list(g) for b, g in r.graphs.items()}
    d0, g0 = eng.counters["decode_steps"], eng.counters["generated_tokens"]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    gen = [eng.add_request(p, sp) for p in ("Why is pod default/api-gateway not ready?", OTHERS[4])]
    emb = [eng.add_request(PROMPT, embed=True)]
    for i in range(6):  # embedding requests keep arriving while the answers decode
        eng.step()
        emb.append(eng.add_request(_ids(20 + i, 700 + i), embed=True))
    while eng.has_work():
        eng.step()
    torch.cuda.synchronize()
    assert captures == [] and eng.stats()["graph_buckets"] == buckets
    assert all(r.graphs[b][i] is g for b, gs in graphs.items() for i, g in enumerate(gs)), "no graph captured again"
    assert eng.counters["generated_tokens"] - g0 == 32 and eng.counters["decode_steps"] > d0
    for s in emb:
        assert s.finish_reason == "embed" and s.output_ids == []
        _close(s.embedding, want(s.prompt_ids))
    for s in gen:
        assert len(s.output_ids) == 16
        _smoke_criterion(eng, s)


def test_gpu_head_spy(served, monkeypatch):
    eng, want = served
    spy = HeadSpy(monkeypatch)
    seqs = [eng.add_request(p, embed=True) for p in (PROMPT, OTHERS[4])]
    while eng.has_work():
        eng.step()
    assert spy.rows == [], "an embedding-only step runs neither the head nor the sampler"
    assert all(s.finish_reason == "embed" for s in seqs)
    gen = eng.add_request(OTHERS[2], SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True))
    while sum(1 for t in gen.output_ids if t >= 0) < 2:
        eng.step()
    del spy.rows[:]
    m0 = eng.counters["mixed_steps"]
    emb = eng.add_request(OTHERS[5], embed=True)
    eng.step()
    assert eng.counters["mixed_steps"] == m0 + 1 and spy.rows == [2], "one decode row + the prompt's last row"
    while eng.has_work():
        eng.step()
    _close(emb.embedding, want(OTHERS[5]))
    assert len(gen.output_ids) == 12
