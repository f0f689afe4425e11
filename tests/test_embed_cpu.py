"""Embedding requests on the CPU: the pooling reference, ``engine.embed`` against an fp32 forward
of the same weights through every scheduling path, the lifecycle of an embedding sequence, the
service's statistics, the refusals, base-model checkpoints, ``POST /v1/embeddings`` and the
data-parallel router."""
import base64
import json
import types

import numpy as np
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, EngineService, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.engine.sequence import SeqStatus
from k8s_llm_monitor_amd.models import AttnMeta, CausalLM
from k8s_llm_monitor_amd.models.reference import fp32_hidden, fp32_logits
from k8s_llm_monitor_amd.ops import reference as ref

MODELS = ["llama-tiny", "qwen3-tiny", "gpt2-tiny"]
GREEDY = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)


def _ids(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 500, (n,), generator=g).tolist()


PROMPT = _ids(40, 0)  # 16 + 16 + 8 with max_prefill_tokens=16: three chunks, two full KV blocks to hit again
OTHERS = [_ids(n, 100 + n) for n in (1, 2, 15, 16, 17, 100, 300)]


def _engine(model="llama-tiny", **kw):
    cfg = dict(model=model, max_num_seqs=8, max_model_len=512, num_blocks=256, use_graphs=False, seed=3)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


def _hidden_rows(model, ids):
    """The final-normed last row of the model's own plain forward (no cache, one sequence): what its
    ``_logits`` is handed.  For the architectures ``fp32_hidden`` does not cover."""
    seen = []
    model._logits = lambda x, rows=None: seen.append(x.float().clone()) or x.new_zeros(x.shape[0], model.cfg.vocab_size)
    try:
        n = len(ids)
        meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32),
                        slot_mapping=torch.full((n,), -1, dtype=torch.int32),
                        cu_seqlens=torch.tensor([0, n], dtype=torch.int32), logits_idx=torch.tensor([n - 1]))
        model.forward(torch.tensor(ids, dtype=torch.int32), meta, None)
    finally:
        del model._logits
    return seen[0]


_REF: dict = {}


def _reference(name, ids=PROMPT):
    """fp32 reference vector of ``ids`` under model ``name`` (seed 3), computed once per module."""
    key = (name, tuple(ids))
    if key not in _REF:
        model = _engine(name).model
        h = _hidden_rows(model, ids) if model.cfg.arch == "gpt2" else fp32_hidden(model, torch.tensor(ids))
        _REF[key] = ref.pool_l2(h, [h.shape[1]])[0].numpy()
    return _REF[key]


def _close(e, want):
    """The project's bf16-against-fp32 bound (smoke() in __graft_entry__.py): 3 % of the scale."""
    assert e is not None and e.dtype == np.float32 and e.shape == want.shape
    err, scale = float(np.abs(e - want).max()), float(np.abs(want).max())
    assert err <= 0.03 * scale, f"max |e - e_ref| = {err:.5f} > 3 % of {scale:.5f}"


# ---------------------------------------------------------------- 1. the reference op

def test_reference_pool_l2():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(6, 24, generator=g)
    x[3] = 0
    dim = [24, 8, 0, 24, -1, 1]
    out = torch.full((6, 24), 7.0)
    got = ops.pool_l2(x, dim, out=out)
    assert got is out and out.dtype == torch.float32
    for r, n in enumerate(dim):
        if n <= 0:
            assert torch.all(out[r] == 7.0), "a row that is no embedding row stays as it was"
            continue
        want = x[r, :n].double() / x[r, :n].double().norm() if r != 3 else torch.zeros(n, dtype=torch.float64)
        assert torch.allclose(out[r, :n].double(), want, rtol=1e-6, atol=0)
        assert torch.all(out[r, n:] == 0)
        if r != 3:
            assert abs(float(out[r].double().norm()) - 1.0) < 1e-6
    assert torch.all(out[3] == 0) and not torch.isnan(out).any(), "a zero row gives zeros, not NaN"
    assert torch.equal(ops.pool_l2(x.bfloat16(), dim)[2], torch.zeros(24)), "a fresh output starts as zeros"
    assert torch.equal(ref.pool_l2(x, dim, out.clone()), out)


def test_pool_l2_refusals():
    x = torch.randn(3, 16)
    for bad in (lambda: ops.pool_l2(x, [16, 17, 1]), lambda: ops.pool_l2(x[0], [16]),
                lambda: ops.pool_l2(x, [16, 16, 16], out=torch.zeros(3, 16, dtype=torch.float64)),
                lambda: ops.pool_l2(x, [16, 16, 16], out=torch.zeros(4, 16)),
                lambda: ops.pool_l2(x, [16, 16, 16], out=torch.zeros(3, 32)[:, :16]),
                lambda: ops.pool_l2(x.half(), [16, 16, 16]), lambda: ops.pool_l2(x, [16])):
        with pytest.raises(ValueError, match="pool_l2"):
            bad()


def test_fp32_logits_is_fp32_hidden_times_the_head():
    model = _engine().model
    ids = torch.tensor(PROMPT)
    h = fp32_hidden(model, ids, [3, 39])
    assert h.shape == (2, model.cfg.d_model) and h.dtype == torch.float32
    want = (h @ model.canonical_head().float().t())[:, : model.cfg.vocab_size]
    assert torch.equal(fp32_logits(model, ids, [3, 39]), want)
    assert torch.equal(fp32_hidden(model, ids), fp32_hidden(model, ids, [39]))


# ---------------------------------------------------------------- 2. engine values

@pytest.mark.parametrize("name", MODELS)
def test_engine_embed_alone_and_among_others(name):
    eng = _engine(name)
    want = _reference(name)
    (e,) = eng.embed([PROMPT])
    _close(e, want)
    assert abs(float(np.linalg.norm(e.astype(np.float64))) - 1.0) < 1e-5
    vecs = eng.embed(OTHERS[:3] + [PROMPT] + OTHERS[3:])
    _close(vecs[3], want)
    for ids, v in zip(OTHERS, vecs[:3] + vecs[4:]):
        if len(ids) in (1, 17, 300):  # the shortest, one past a block, the longest: each its own vector
            _close(v, _reference(name, ids))


@pytest.mark.parametrize("name", MODELS)
def test_engine_embed_in_three_chunks(name):
    eng = _engine(name, max_prefill_tokens=16)
    (e,) = eng.embed([PROMPT])
    assert eng.counters["prefill_steps"] == 3 and eng.runner.n_steps["prefill_tokens"] == len(PROMPT)
    _close(e, _reference(name))


@pytest.mark.parametrize("name", MODELS)
def test_engine_embed_prefix_cache_hit(name):
    eng = _engine(name)
    first, second = eng.embed([PROMPT])[0], eng.embed([PROMPT])[0]
    # the second request attends the first one's two full blocks and computes the remaining tokens only
    assert eng.runner.n_steps["prefill_context_tokens"] == 32
    _close(first, _reference(name))
    _close(second, _reference(name))
    once_more = eng.embed([PROMPT[:32]])[0]  # every block cached: one token is still computed
    _close(once_more, _reference(name, PROMPT[:32]))


@pytest.mark.parametrize("pipeline", [True, False])
@pytest.mark.parametrize("name", MODELS)
def test_engine_embed_in_a_mixed_step(name, pipeline):
    eng = _engine(name, pipeline=pipeline)
    gen = [eng.add_request(p, GREEDY) for p in OTHERS[2:4]]
    while not all(len(s.output_ids) >= 2 for s in gen):
        eng.step()
    m0 = eng.counters["mixed_steps"]
    seq = eng.add_request(PROMPT, embed=True)
    while eng.has_work():
        eng.step()
    assert eng.counters["mixed_steps"] == m0 + 1, "the embedding prompt rode along a decode step"
    assert seq.finish_reason == "embed" and all(len(s.output_ids) == 8 for s in gen)
    _close(seq.embedding, _reference(name))


# ---------------------------------------------------------------- 3. dimensions

@pytest.mark.parametrize("name", MODELS)
def test_dimensions_is_the_renormalised_head_of_the_full_vector(name):
    eng = _engine(name)
    full, cut = eng.embed([PROMPT])[0], eng.embed([PROMPT], dim=8)[0]
    assert cut.shape == (8,) and cut.dtype == np.float32
    want = full[:8].astype(np.float64) / np.linalg.norm(full[:8].astype(np.float64))
    # full = x / |x| and cut = x[:8] / |x[:8]| in fp32, both from the same row x: a few roundings apart
    assert np.abs(cut - want).max() <= 8 * 2.0 ** -24 * np.abs(want).max()
    assert eng.add_request(PROMPT, embed=0).embed_dim == eng.model_cfg.d_model
    assert eng.add_request(PROMPT, embed=True).embed_dim == eng.model_cfg.d_model


# ---------------------------------------------------------------- 4. lifecycle

class HeadSpy:
    """Counts the rows of every LM-head call (``CausalLM._logits``)."""

    def __init__(self, monkeypatch):
        self.rows = []
        orig = CausalLM._logits

        def spy(model, x, rows=None):
            self.rows.append(int(x.shape[0]) if rows is None else int(rows))
            return orig(model, x, rows)

        monkeypatch.setattr(CausalLM, "_logits", spy)


@pytest.mark.parametrize("pipeline", [True, False])
def test_lifecycle_and_no_head_call(monkeypatch, pipeline):
    eng = _engine(pipeline=pipeline)
    free0 = eng.stats()["kv_blocks_free"]
    assert not eng.stats()["embed_enabled"] and not eng.runner.embed_on
    spy = HeadSpy(monkeypatch)
    seqs = [eng.add_request(p, embed=True) for p in (PROMPT, OTHERS[4])]
    while eng.has_work():
        eng.step()
    assert spy.rows == [], "an embedding-only step runs neither the head nor the sampler"
    for s in seqs:
        assert s.status == SeqStatus.FINISHED and s.finish_reason == "embed" and s.output_ids == []
        assert not s.prefilled and s.t_first_token == s.t_finish and s.embedding.shape == (eng.model_cfg.d_model,)
    st = eng.stats()
    assert st["decode_steps"] == 0 and st["generated_tokens"] == 0 and st["kv_blocks_free"] == free0
    assert st["embed_enabled"] and st["embed_requests"] == 2 and st["embed_tokens"] == len(PROMPT) + len(OTHERS[4])
    assert st["requests"] == st["finished"] == 2 and st["running"] == st["waiting"] == 0
    # a mixed step: the head runs over its rows exactly as it does without the embedding request
    gen = eng.add_request(OTHERS[2], GREEDY)
    while len(gen.output_ids) < 2:
        eng.step()
    del spy.rows[:]
    emb = eng.add_request(OTHERS[5], embed=True)
    eng.step()
    assert spy.rows[0] == 2, "one decode row + the embedding prompt's last row"
    while eng.has_work():
        eng.step()
    assert emb.finish_reason == "embed" and emb.output_ids == [] and len(gen.output_ids) == 8
    assert eng.stats()["generated_tokens"] == 8 and eng.stats()["kv_blocks_free"] == free0


def test_deadline_gives_no_embedding():
    eng = _engine(max_prefill_tokens=16)
    seq = eng.add_request(PROMPT, embed=True, deadline=0.0)  # long past
    while eng.has_work():
        eng.step()
    assert seq.finish_reason == "deadline" and seq.embedding is None and seq.output_ids == []
    assert eng.counters["deadline_stops"] == 1


# ---------------------------------------------------------------- 5. no effect on generation

def test_generation_is_unchanged_by_embedding_requests():
    prompts = [OTHERS[2], OTHERS[3], OTHERS[4], PROMPT]
    want = [s.output_ids for s in _engine(dtype="float32", max_num_seqs=16).generate(prompts, GREEDY)]
    eng = _engine(dtype="float32", max_num_seqs=16)
    gen = [eng.add_request(p, GREEDY) for p in prompts[:2]]
    emb = [eng.add_request(_ids(20 + i, 50 + i), embed=True) for i in range(4)]
    gen += [eng.add_request(p, GREEDY) for p in prompts[2:]]
    eng.step()
    emb += [eng.add_request(_ids(30 + i, 60 + i), embed=True) for i in range(4)]  # these join running decodes
    while eng.has_work():
        eng.step()
    assert [s.output_ids for s in gen] == want
    assert all(s.finish_reason == "embed" and s.embedding is not None for s in emb)


# ---------------------------------------------------------------- 6. statistics

def test_service_records_no_answer_length_and_no_tpot_sample():
    eng = _engine()
    svc = EngineService(eng)
    try:
        futs = [svc.submit(p, None, embed=True) for p in OTHERS[:5]] + [svc.submit("node-1 NotReady", embed=8)]
        res = [f.result(timeout=120) for f in futs]
        assert all(text is None and seq.finish_reason == "embed" for text, seq in res)
        assert res[-1][1].embedding.shape == (8,)
        assert len(svc.answer_lens.lens) == 0 and len(svc.tpot.samples) == 0 and len(eng.step_samples) == 0
        assert svc._expected_rem(res[0][1]) == 0
        st = svc.stats()
        assert st["embed_requests"] == 6 and st["generated_tokens"] == 0 and st["decode_steps"] == 0
        # a generation request is still recorded
        text, seq = svc.submit("node-1 NotReady", SamplingParams(max_tokens=3, temperature=0.0)).result(timeout=120)
        assert isinstance(text, str) and len(seq.output_ids) <= 3 and len(svc.answer_lens.lens) == 1
    finally:
        svc.close()


# ---------------------------------------------------------------- 7. refusals

def test_refusals():
    eng = _engine(max_model_len=64)
    d = eng.model_cfg.d_model
    for bad in (-1, d + 1, 8.0, "8", [8]):
        with pytest.raises(ValueError, match="embed must be"):
            eng.add_request(PROMPT, embed=bad)
    for p in (SamplingParams(logprobs=True), SamplingParams(top_logprobs=2), SamplingParams(guide={"regex": "a+"}),
              SamplingParams(adapter="a"), SamplingParams(repetition_penalty=1.1),
              SamplingParams(presence_penalty=0.5), SamplingParams(frequency_penalty=0.5)):
        with pytest.raises(ValueError, match="embedding request takes no"):
            eng.add_request(PROMPT, p, embed=True)
    with pytest.raises(ValueError, match="empty prompt"):
        eng.add_request([], embed=True)
    limit = eng.runner.max_len - 1
    with pytest.raises(ValueError, match="exceeds the limit"):
        eng.add_request(_ids(limit + 1, 9), embed=True)
    ok = eng.add_request(_ids(limit, 9), embed=True)  # never trimmed in the middle, and it fits
    assert len(ok.prompt_ids) == limit
    assert len(eng.add_request(_ids(limit + 1, 9)).prompt_ids) < limit, "generation prompts are still trimmed"
    assert eng.counters["embed_requests"] == 1
    while eng.has_work():
        eng.step()
    assert ok.embedding is not None
    eng.ps = types.SimpleNamespace(tp_size=2, tp_rank=0)  # as a TP leader sees itself
    with pytest.raises(ValueError, match="tensor parallelism"):
        eng.add_request(PROMPT, embed=True)
    eng.add_request(PROMPT)  # generation requests are not affected


# ---------------------------------------------------------------- 8. the loader

def _hf_qwen3_base():
    transformers = pytest.importorskip("transformers")  # the two loader tests alone need it
    torch.manual_seed(0)
    cfg = transformers.Qwen3Config(vocab_size=320, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                                   max_position_embeddings=256, rope_theta=1e6, rms_norm_eps=1e-6,
                                   tie_word_embeddings=False, bos_token_id=1, eos_token_id=2)
    hf = transformers.Qwen3Model(cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # every parameter random: HF inits the norms to 1
        for _, p in hf.named_parameters():
            if p.dim() == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
    return hf.float().eval()


def test_base_model_checkpoint_serves_embeddings_only(tmp_path):
    from safetensors import safe_open

    hf = _hf_qwen3_base()
    hf.save_pretrained(tmp_path, safe_serialization=True)
    with safe_open(str(tmp_path / "model.safetensors"), "pt") as f:
        names = set(f.keys())
    assert "embed_tokens.weight" in names and "norm.weight" in names and "lm_head.weight" not in names
    assert not any(n.startswith("model.") for n in names)
    eng = LLMEngine(EngineConfig(weights=str(tmp_path), max_num_seqs=2, max_model_len=128, num_blocks=32,
                                 use_graphs=False, dtype="float32"), device="cpu")
    assert eng.model.has_head is False and eng.model_cfg.qk_norm
    ids = [1, 17, 33, 250, 5, 99, 140, 7, 61, 200, 3, 45]
    (e,) = eng.embed([ids])
    with torch.no_grad():
        h = hf(torch.tensor([ids])).last_hidden_state[0, -1].float()
    want = (h / h.norm()).numpy()
    err = float(np.abs(e - want).max())
    assert err <= 2e-3 * float(np.abs(want).max()), f"max |e - hf| = {err}"
    with pytest.raises(ValueError, match="embedding-only checkpoint"):
        eng.add_request(ids, SamplingParams(max_tokens=2))
    with pytest.raises(ValueError, match="embedding-only checkpoint"):
        eng.generate([ids])


def test_causal_lm_checkpoint_still_generates(tmp_path):
    torch.manual_seed(0)
    base = _hf_qwen3_base()
    import transformers

    hf = transformers.Qwen3ForCausalLM(base.config)
    hf.model.load_state_dict(base.state_dict())
    with torch.no_grad():  # decisive logits
        for p in hf.parameters():
            if p.dim() == 2:
                p.mul_(3.0)
    hf = hf.float().eval()
    hf.save_pretrained(tmp_path, safe_serialization=True)
    eng = LLMEngine(EngineConfig(weights=str(tmp_path), max_num_seqs=2, max_model_len=128, num_blocks=32,
                                 use_graphs=False, dtype="float32"), device="cpu")
    assert eng.model.has_head is True
    ids = [1, 17, 33, 250, 5, 99, 140, 7, 61, 200, 3, 45]
    (s,) = eng.generate([ids], SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))
    with torch.no_grad():
        out = hf.generate(torch.tensor([ids]), max_new_tokens=6, do_sample=False,
                          attention_mask=torch.ones(1, len(ids), dtype=torch.long))[0, len(ids):].tolist()
    assert s.output_ids == out
    (e,) = eng.embed([ids])  # and the same checkpoint embeds
    with torch.no_grad():
        h = hf.model(torch.tensor([ids])).last_hidden_state[0, -1].float()
    want = (h / h.norm()).numpy()
    assert float(np.abs(e - want).max()) <= 2e-3 * float(np.abs(want).max())


# ---------------------------------------------------------------- 9. HTTP

def _monitor(backend, **llm):
    from k8s_llm_monitor_amd.monitor.app import build_monitor
    from k8s_llm_monitor_amd.monitor.cluster.fake import FakeCluster
    from k8s_llm_monitor_amd.monitor.config import from_dict

    m = build_monitor(from_dict({"llm": {"provider": "none", **llm}}), backend=FakeCluster.build(seed=2),
                      start_manager=False, llm=True)
    m.analysis.backend = backend
    return m


def _post(app, **body):
    return app.handle("POST", "/v1/embeddings", json.dumps(body).encode())


@pytest.fixture(scope="module")
def served():
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend

    eng = _engine(max_model_len=128)
    svc = EngineService(eng)
    be = LocalEngineBackend(svc, max_tokens=4, temperature=0.0, timeout_s=60.0)
    yield eng, svc, be, _monitor(be, embed_max_inputs=5).app
    svc.close()


def test_config_keys():
    from k8s_llm_monitor_amd.monitor.config import from_dict

    c = from_dict({})
    assert c.llm.embed_append_eos is False and c.llm.embed_max_inputs == 64
    c = from_dict({"llm": {"embed_append_eos": True, "embed_max_inputs": 5}})
    assert c.llm.embed_append_eos is True and c.llm.embed_max_inputs == 5


def test_http_input_shapes_order_and_usage(served):
    eng, svc, be, app = served
    text, text2 = "pod default/api-gateway CrashLoopBackOff", "node-003 NotReady since 12:04"
    ids, ids2 = eng.tokenizer.encode(text), eng.tokenizer.encode(text2)
    w1, w2 = _reference("llama-tiny", ids), _reference("llama-tiny", ids2)
    # the two texts' vectors are far apart next to the bound, so a vector in the wrong place shows
    assert np.abs(w1 - w2).max() > 0.2 * np.abs(w1).max()

    def data(r):
        assert r.code == 200, r.body
        d = json.loads(r.body)
        assert d["object"] == "list" and d["model"] == "llama-tiny"
        assert [x["index"] for x in d["data"]] == list(range(len(d["data"])))
        assert all(x["object"] == "embedding" for x in d["data"])
        return d, [np.asarray(x["embedding"], dtype=np.float32) for x in d["data"]]

    d, (v,) = data(_post(app, input=text))
    _close(v, w1)
    assert d["usage"] == {"prompt_tokens": len(ids), "total_tokens": len(ids)}
    d, (v,) = data(_post(app, input=ids, model="whatever"))
    _close(v, w1)
    d, vs = data(_post(app, input=[text2, text, text2]))
    for v, w in zip(vs, (w2, w1, w2)):
        _close(v, w)
    assert d["usage"]["prompt_tokens"] == d["usage"]["total_tokens"] == 2 * len(ids2) + len(ids)
    d, vs = data(_post(app, input=[ids2, ids]))
    _close(vs[0], w2)
    _close(vs[1], w1)


def test_http_dimensions_and_base64(served):
    eng, svc, be, app = served
    r = _post(app, input=["a b c", "d e"], dimensions=16)
    f = [x["embedding"] for x in json.loads(r.body)["data"]]
    assert r.code == 200 and [len(v) for v in f] == [16, 16]
    assert all(abs(np.linalg.norm(np.asarray(v)) - 1.0) < 1e-5 for v in f)
    r64 = _post(app, input=["a b c", "d e"], dimensions=16, encoding_format="base64")
    assert r64.code == 200
    for x, v in zip(json.loads(r64.body)["data"], f):
        raw = base64.b64decode(x["embedding"])
        assert len(raw) == 64 and np.frombuffer(raw, dtype="<f4").tolist() == v, "the same bits as the float reply"
    assert _post(app, input="a b c", encoding_format="float").code == 200


def test_http_append_eos(served):
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend

    eng, svc, be, app = served
    be2 = LocalEngineBackend(svc, timeout_s=60.0, embed_append_eos=True)
    ids = eng.tokenizer.encode("a b c")
    assert ids[0] == eng.model_cfg.bos_id
    (v,), n = be2.embed(["a b c"])
    (w,), _ = be.embed([ids + [eng.model_cfg.eos_ids[0]]])
    assert n == len(ids) + 1 and np.array_equal(v, w)
    (u,), n = be2.embed([ids])  # token ids are taken as given
    assert n == len(ids) and not np.array_equal(u, v)


def test_http_400s_and_405(served):
    eng, svc, be, app = served
    n0 = eng.counters["requests"]
    V, d = eng.model_cfg.vocab_size, eng.model_cfg.d_model
    long_ids = _ids(128, 4)
    for body in ({}, {"input": ""}, {"input": []}, {"input": None}, {"input": 7}, {"input": ["a", ""]},
                 {"input": [[1, 2], []]}, {"input": ["a", 3]}, {"input": [[1, 2], "a", {}]},
                 {"input": ["a"] * 6}, {"input": [1, V]}, {"input": [[1, -1]]}, {"input": [[1, 2.5]]},
                 {"input": [[1, True]]}, {"input": long_ids}, {"input": " ".join(str(i * 7919) for i in range(200))},
                 {"input": "a", "dimensions": 0}, {"input": "a", "dimensions": d + 1},
                 {"input": "a", "dimensions": "8"}, {"input": "a", "dimensions": 8.0},
                 {"input": "a", "dimensions": True}, {"input": "a", "encoding_format": "hex"}):
        r = _post(app, **body)
        assert r.code == 400 and len(r.body.strip()) > 0, (body, r.code, r.body)
    assert app.handle("POST", "/v1/embeddings", b"not json").code == 400
    assert eng.counters["requests"] == n0, "nothing invalid reached the engine"
    assert _post(app, input=["a"] * 5).code == 200  # llm.embed_max_inputs itself is fine
    for method in ("GET", "PUT", "DELETE"):
        assert app.handle(method, "/v1/embeddings").code == 405


def test_http_backend_without_embed_and_engine_refusal(served):
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend, OpenAIBackend, RuleBackend

    assert not hasattr(OpenAIBackend, "embed") and not hasattr(RuleBackend, "embed")
    r = _post(_monitor(RuleBackend()).app, input="a")
    assert r.code == 400 and b"no embeddings" in r.body
    eng = _engine()
    eng.ps = types.SimpleNamespace(tp_size=2, tp_rank=0)  # what the engine refuses with ValueError is a 400
    svc = EngineService(eng)
    try:
        r = _post(_monitor(LocalEngineBackend(svc, timeout_s=60.0)).app, input="a")
        assert r.code == 400 and b"tensor parallelism" in r.body
    finally:
        svc.close()


def test_http_503_and_504(served):
    from k8s_llm_monitor_amd.engine import EngineOverloaded
    from k8s_llm_monitor_amd.llm.service import AnswerBudgetExceeded

    class Busy:
        provider = model = "stub"

        def __init__(self, exc):
            self.exc = exc

        def embed(self, inputs, dimensions=None):
            raise self.exc

    assert _post(_monitor(Busy(EngineOverloaded("request queue full"))).app, input="a").code == 503
    assert _post(_monitor(Busy(AnswerBudgetExceeded("late"))).app, input="a").code == 504
    assert _post(_monitor(Busy(RuntimeError("engine step failed"))).app, input="a").code == 500


def test_first_failure_cancels_the_rest():
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend

    class Svc:
        """Two futures: the first fails, the second never resolves."""

        def __init__(self, engine):
            from concurrent.futures import Future

            self.engine, self.futs, self.cancelled = engine, [Future(), Future()], []
            self.futs[0].set_exception(ValueError("refused"))
            self._it = iter(self.futs)

        def submit(self, *a, **kw):
            return next(self._it)

        def cancel(self, fut):
            self.cancelled.append(fut)
            return fut.cancel()

    svc = Svc(_engine())
    with pytest.raises(ValueError, match="refused"):
        LocalEngineBackend(svc, timeout_s=60.0).embed(["a", "b"])
    assert svc.cancelled == [svc.futs[1]]


# ---------------------------------------------------------------- 10. the data-parallel router

def test_router_returns_the_in_process_vector():
    from k8s_llm_monitor_amd.engine.dp import ReplicaRouter
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend

    cfg = dict(model="llama-tiny", max_num_seqs=4, max_model_len=256, num_blocks=64, use_graphs=False, seed=7)
    svc = EngineService(LLMEngine(EngineConfig(**cfg), device="cpu"))
    try:
        _, seq = svc.submit(PROMPT, None, embed=True).result(timeout=120)
        _, seq8 = svc.submit("node-9 NotReady", None, embed=8).result(timeout=120)
    finally:
        svc.close()
    router = ReplicaRouter(EngineConfig(**cfg), ["cpu"])
    try:
        text, rs = router.submit(PROMPT, None, embed=True).result(timeout=120)
        assert text is None and rs.finish_reason == "embed" and rs.output_ids == [] and rs.embed_dim == 256
        assert rs.embedding.dtype == np.float32 and np.array_equal(rs.embedding, seq.embedding)
        (v,), n = LocalEngineBackend(router, timeout_s=120).embed(["node-9 NotReady"], dimensions=8)
        assert np.array_equal(v, seq8.embedding) and n == len(seq8.prompt_ids)
        st = router.stats()
        assert st["finished"] == 2 and st["generated_tokens"] == 0
    finally:
        router.close()
