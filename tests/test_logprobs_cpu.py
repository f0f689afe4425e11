"""Token log-probabilities without a GPU: the reference against fp64, the packed record of the
CPU path, the CPU engine (pipelined resolution, a stop, a neighbour that does not ask), the
refusals and the HTTP surface."""
import json
import types

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.ops import reference as ref

SHAPES = [(3, 50257), (5, 128256), (128, 32000), (2, 1000), (1, 16)]
N_TOP = 20
# |fp32 logprob - fp64| on these inputs: the result's half ulp (2e-6 at magnitude <= 40), an fp32
# tree sum of V <= 2^17 terms (a few log2(V) * 2^-24 relative) and the exponential (1e-6 relative)
# come to about 1e-5; torch's fp32 log_softmax measures 4e-6 to 7e-6 here.  1e-4 is ~7x that.
LP_TOL = 1e-4


def make_logits(B, V, seed=0):
    """bf16 [B, V]: multiples of 1/16 in [-8, 8] (exact in bf16, many ties at every value), with
    entries 5..8 of row 0 -inf."""
    g = torch.Generator().manual_seed(1000 * seed + V + B)
    x = (torch.randint(-128, 129, (B, V), generator=g).float() / 16).to(torch.bfloat16)
    x[0, 5:9] = float("-inf")
    return x


def fp64_logprobs(row):
    """(lps fp64 [V], ids of the stable descending sort) of one row."""
    x = row.double()
    return torch.log_softmax(x, -1), torch.sort(x, descending=True, stable=True).indices


def check_entry(entry, row, tok, n, tol=LP_TOL):
    """One unpacked entry (lp, [(id, lp), ...]) against fp64 over ``row``; returns the largest
    error seen on finite values."""
    lps64, order = fp64_logprobs(row)
    V = row.numel()
    lp, top = entry
    err = abs(lp - float(lps64[tok]))
    assert err <= tol, (lp, float(lps64[tok]))
    k = min(n, V)
    assert [i for i, _ in top] == order[:k].tolist()
    for i, v in top:
        w = float(lps64[i])
        if w == float("-inf"):
            assert v == float("-inf")
        else:
            assert abs(v - w) <= tol, (i, v, w)
            err = max(err, abs(v - w))
    return err


# ---------------------------------------------------------------- 1. the reference against fp64

@pytest.mark.parametrize("B,V", SHAPES)
def test_reference_matches_fp64(B, V):
    x = make_logits(B, V)
    g = torch.Generator().manual_seed(V)
    toks = torch.randint(0, V, (B,), generator=g).tolist()
    for b in sorted({0, 1 % B, B // 2, B - 1}):
        lp, ids, lps = ref.token_logprobs(x[b], toks[b], N_TOP)
        assert ids.dtype == torch.int32 and lps.dtype == torch.float32 and ids.numel() == N_TOP == lps.numel()
        k = min(N_TOP, V)
        assert ids[k:].tolist() == [-1] * (N_TOP - k) and bool((lps[k:] == float("-inf")).all())
        check_entry((lp, list(zip(ids[:k].tolist(), lps[:k].tolist()))), x[b], toks[b], N_TOP)


def test_reference_ties_go_to_the_lower_index_and_minus_inf_may_be_an_alternative():
    x = torch.tensor([1.0, 3.0, 3.0, float("-inf"), 3.0, float("-inf")])
    lp, ids, lps = ref.token_logprobs(x, 2, 6)
    assert ids.tolist() == [1, 2, 4, 0, 3, 5]
    assert lps[4:].tolist() == [float("-inf")] * 2
    assert lp == pytest.approx(float(torch.log_softmax(x.double(), -1)[2]), abs=1e-6)


# ---------------------------------------------------------------- 2. ops.token_logprobs on the CPU

def test_ops_token_logprobs_cpu_packed_layout():
    assert ops.LP_MAX_TOP == 20 and ops.LP_WIDTH == 41
    V = 16
    x = make_logits(6, V)
    tok = torch.tensor([3, 7, 0, 15, V, -1], dtype=torch.int32)  # the last two out of range
    want = torch.tensor([5, -1, 0, 20, 1, 0], dtype=torch.int32)
    sentinel = 0x5A5A5A5A
    out = torch.full((6, ops.LP_WIDTH), sentinel, dtype=torch.int32)
    got = ops.token_logprobs(x, tok, want, out=out)
    assert got is out
    assert bool((out[1] == sentinel).all())  # want = -1: untouched
    for b in (0, 2, 3):
        lp, ids, lps = ref.token_logprobs(x[b], int(tok[b]), max(int(want[b]), 0))
        rec = out[b]
        assert rec[:1].view(torch.float32).item() == lp
        n = int(want[b])
        k = min(n, V)
        assert rec[1:1 + n].view(torch.float32).tolist() == lps.tolist()
        assert rec[21:21 + n].tolist() == ids.tolist()
        assert rec[21 + k:].tolist() == [-1] * (20 - k)  # n > V pads with (-1, -inf)
        assert bool((rec[1 + k:21].view(torch.float32) == float("-inf")).all())
        e = ops.unpack_logprobs(rec)
        assert e[0] == lp and e[1] == list(zip(ids[:k].tolist(), lps[:k].tolist()))
    assert ops.unpack_logprobs(out[2])[1] == []  # want = 0: no alternatives
    for b in (4, 5):  # a token outside [0, V): NaN
        lp, top = ops.unpack_logprobs(out[b])
        assert lp != lp and len(top) == int(want[b])
    fresh = ops.token_logprobs(x.float(), tok, want)
    assert fresh.shape == (6, ops.LP_WIDTH) and torch.equal(fresh[0], out[0])


# ---------------------------------------------------------------- 3. the engine on the CPU

PROMPTS = ["kube-system coredns CrashLoopBackOff", "MEM=95.9% [资源压力]", "node-003 NotReady since 12:04"]


def _engine(**kw):
    cfg = dict(model="llama-tiny", max_num_seqs=4, max_model_len=256, num_blocks=64, use_graphs=False,
               dtype="float32", seed=5)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


class ForwardSpy:
    """Records the logits row behind every token a step samples, keyed (seq_id, index in
    output_ids): wraps the model's forward and the runner's two launch entry points.  The
    yardstick of the engine tests, not the code under test."""

    def __init__(self, eng):
        self.rows = {}
        self._keys = None
        r = eng.runner
        fwd, pl, dl = r.model.forward, r.prefill_launch, r.decode_launch

        def forward(ids, meta, kv):
            out = fwd(ids, meta, kv)
            for i, key in enumerate(self._keys or []):
                self.rows[key] = out[i].detach().float().cpu().clone()
            return out

        def prefill_launch(seqs, decode=None):
            # a chunk short of its prompt's end is overwritten by the chunk that completes it
            self._keys = [(q.seq_id, len(q.output_ids)) for q in list(decode or []) + list(seqs)]
            try:
                return pl(seqs, decode)
            finally:
                self._keys = None

        def decode_launch(seqs, src_rows=None, publish=None):
            self._keys = [(q.seq_id, len(q.output_ids)) for q in seqs]
            try:
                return dl(seqs, src_rows, publish=publish)
            finally:
                self._keys = None

        r.model.forward, r.prefill_launch, r.decode_launch = forward, prefill_launch, decode_launch


def _params():
    return [SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True, logprobs=True, top_logprobs=5),
            SamplingParams(max_tokens=8, temperature=0.8, ignore_eos=True, logprobs=True, top_logprobs=0),
            SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)]


def _run(eng, params):
    seqs = [eng.add_request(p, sp) for p, sp in zip(PROMPTS, params)]
    while eng.has_work():
        eng.step()
    return seqs


def check_sequence(seq, spy, n_top):
    assert len(seq.output_logprobs) == len(seq.output_ids)
    for j, (tok, entry) in enumerate(zip(seq.output_ids, seq.output_logprobs)):
        row = spy.rows[(seq.seq_id, j)]
        assert len(entry[1]) == n_top
        check_entry(entry, row, tok, n_top)
        want = ref.token_logprobs(row, tok, n_top)
        assert abs(entry[0] - want[0]) <= LP_TOL and [i for i, _ in entry[1]] == want[1].tolist()


@pytest.mark.parametrize("pipeline", [True, False])
def test_engine_cpu_entries_match_the_recorded_logits(pipeline):
    eng = _engine(pipeline=pipeline)
    assert eng.stats()["logprobs_enabled"] is False
    spy = ForwardSpy(eng)
    seqs = _run(eng, _params())
    assert eng.stats()["logprobs_enabled"] is True
    assert [len(s.output_ids) for s in seqs] == [8, 8, 8]
    check_sequence(seqs[0], spy, 5)
    check_sequence(seqs[1], spy, 0)
    assert seqs[2].output_logprobs is None
    # the feature does not touch sampling: the same engine without logprobs draws the same tokens
    plain = _run(_engine(pipeline=pipeline), [SamplingParams(max_tokens=8, temperature=sp.temperature, ignore_eos=True)
                                              for sp in _params()])
    assert [s.output_ids for s in plain] == [s.output_ids for s in seqs]
    assert all(s.output_logprobs is None for s in plain)


def test_engine_cpu_stop_under_pipelined_resolution_trims_both_lists():
    # sampled at temperature 1 (the draws are a function of the seed and the step), so that the
    # answer does not repeat one token: stop at the first token, from the third on, that is new
    free = _run(_engine(), [SamplingParams(max_tokens=8, temperature=1.0, ignore_eos=True)])[0].output_ids
    k = next(j for j in range(2, 8) if free[j] not in free[:j] and free[j] not in (0, 1, 2))
    stop = free[k]
    eng = _engine()
    spy = ForwardSpy(eng)
    sp = SamplingParams(max_tokens=8, temperature=1.0, logprobs=True, top_logprobs=2, stop_token_ids=(stop,))
    seq = eng.add_request(PROMPTS[0], sp)
    while eng.has_work():
        eng.step()
    assert seq.finish_reason == "stop" and seq.output_ids == free[:len(seq.output_ids)]
    assert len(seq.output_ids) <= k + 1 and len(seq.output_ids) >= 2
    assert (seq.seq_id, len(seq.output_ids)) in spy.rows  # a step was launched past the stop
    check_sequence(seq, spy, 2)


def test_engine_cpu_preempted_sequence_keeps_its_entries():
    eng = _engine()
    spy = ForwardSpy(eng)
    sp = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True, logprobs=True, top_logprobs=3)
    seq = eng.add_request(PROMPTS[0], sp)
    while len([t for t in seq.output_ids if t >= 0]) < 4:
        eng.step()
    if eng._inflight is not None:
        eng._resolve()
    kept = list(seq.output_logprobs)
    eng.sched._preempt(seq)
    eng.sched.running.remove(seq)
    while eng.has_work():
        eng.step()
    assert len(seq.output_ids) == 8 and seq.output_logprobs[:len(kept)] == kept
    check_sequence(seq, spy, 3)


# ---------------------------------------------------------------- 4. refusals

def test_engine_refuses_invalid_logprob_requests():
    eng = _engine()
    with pytest.raises(ValueError, match="top_logprobs"):
        eng.add_request("x", SamplingParams(logprobs=True, top_logprobs=21))
    with pytest.raises(ValueError, match="needs logprobs"):
        eng.add_request("x", SamplingParams(top_logprobs=3))
    assert eng.stats()["logprobs_enabled"] is False
    eng.ps = types.SimpleNamespace(tp_size=2, tp_rank=0)
    with pytest.raises(ValueError, match="tensor parallelism"):
        eng.add_request("x", SamplingParams(logprobs=True))
    eng.add_request("x", SamplingParams())  # requests that do not ask are not affected


# ---------------------------------------------------------------- 5. HTTP

def _monitor(backend):
    from k8s_llm_monitor_amd.monitor.app import build_monitor
    from k8s_llm_monitor_amd.monitor.cluster.fake import FakeCluster
    from k8s_llm_monitor_amd.monitor.config import from_dict

    m = build_monitor(from_dict({"llm": {"provider": "none"}}), backend=FakeCluster.build(seed=2),
                      start_manager=False, llm=True)
    m.analysis.backend = backend
    return m


def _chat(app, **fields):
    body = {"messages": [{"role": "user", "content": "hi"}], **fields}
    return app.handle("POST", "/v1/chat/completions", json.dumps(body).encode())


class _Stub:
    provider, model = "stub", "stub"
    ENTRIES = [{"token": "o", "logprob": -0.5, "bytes": [111], "top_logprobs": []},
               {"token": "k", "logprob": -2.0, "bytes": [107], "top_logprobs": []},
               {"token": "!", "logprob": -0.25, "bytes": [33], "top_logprobs": []}]

    def __init__(self):
        self.calls = []

    def count_tokens(self, text):
        return len(text)

    def generate(self, prompt, **kw):
        from k8s_llm_monitor_amd.llm.service import GenResult

        self.calls.append(kw)
        g = GenResult(text="ok!", model="stub", provider="stub", prompt_tokens=1, completion_tokens=3,
                      latency_ms=0.0, ttft_ms=0.0, finish_reason="stop")
        if kw.get("logprobs"):
            g["logprobs"] = [dict(e) for e in self.ENTRIES]
        return g


def test_chat_route_returns_logprobs_from_the_cpu_engine():
    from k8s_llm_monitor_amd.engine import EngineService
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend

    eng = _engine()
    svc = EngineService(eng)
    try:
        app = _monitor(LocalEngineBackend(svc, max_tokens=4, temperature=0.0, timeout_s=60.0)).app
        plain = _chat(app, max_tokens=4)
        assert plain.code == 200 and "logprobs" not in json.loads(plain.body)["choices"][0]
        r = _chat(app, max_tokens=4, logprobs=True, top_logprobs=3)
        assert r.code == 200
        d = json.loads(r.body)
        content = d["choices"][0]["logprobs"]["content"]
        assert len(content) == d["usage"]["completion_tokens"] > 0
        tok = eng.tokenizer
        for e in content:
            assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
            assert e["logprob"] <= 0.0 and isinstance(e["bytes"], list) and len(e["top_logprobs"]) == 3
            lps = [t["logprob"] for t in e["top_logprobs"]]
            assert lps == sorted(lps, reverse=True) and e["logprob"] <= lps[0]
            assert all(bytes(t["bytes"]).decode("utf-8", errors="replace") == t["token"] for t in e["top_logprobs"])
            assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"]
        # greedy at temperature 0: the drawn token is the most likely alternative
        assert all(e["top_logprobs"][0]["logprob"] == e["logprob"] for e in content)
        assert tok.token_bytes(65) == b"A" and tok.token_bytes(tok.eos_id) == tok._token_bytes(tok.eos_id, False)
        only = json.loads(_chat(app, max_tokens=4, logprobs=True).body)["choices"][0]["logprobs"]["content"]
        assert [e["logprob"] for e in only] == [e["logprob"] for e in content]
        assert all(e["top_logprobs"] == [] for e in only)
    finally:
        svc.close()


def test_chat_route_refuses_invalid_logprob_fields():
    be = _Stub()
    app = _monitor(be).app
    assert _chat(app, logprobs=True, top_logprobs=20).code == 200
    assert (be.calls[-1]["logprobs"], be.calls[-1]["top_logprobs"]) == (True, 20)
    assert _chat(app, logprobs=False).code == 200 and "logprobs" not in be.calls[-1]
    n = len(be.calls)
    for bad in ({"logprobs": 1}, {"logprobs": "true"}, {"logprobs": True, "top_logprobs": 21},
                {"logprobs": True, "top_logprobs": -1}, {"logprobs": True, "top_logprobs": 2.0},
                {"logprobs": True, "top_logprobs": True}, {"top_logprobs": 3}, {"logprobs": False, "top_logprobs": 3}):
        assert _chat(app, **bad).code == 400, bad
    assert len(be.calls) == n  # nothing invalid reached the backend


def test_chat_route_answers_400_when_the_engine_cannot_compute_logprobs():
    from k8s_llm_monitor_amd.engine import EngineService
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend

    eng = _engine()
    eng.ps = types.SimpleNamespace(tp_size=2, tp_rank=0)  # as a TP leader sees itself
    svc = EngineService(eng)
    try:
        app = _monitor(LocalEngineBackend(svc, max_tokens=4, temperature=0.0, timeout_s=60.0)).app
        r = _chat(app, logprobs=True, max_tokens=4)
        assert r.code == 400 and b"tensor parallelism" in r.body
        assert _chat(app, max_tokens=4).code == 200
    finally:
        svc.close()


def test_query_and_analyze_store_the_mean_and_min_logprob():
    be = _Stub()
    m = _monitor(be)
    post = lambda path, body: m.app.handle("POST", path, json.dumps(body).encode())  # noqa: E731
    r = post("/api/v1/query", {"question": "why?", "logprobs": True})
    assert r.code == 200 and be.calls[-1].get("logprobs") is True
    res = json.loads(r.body)["result"]
    vals = [e["logprob"] for e in _Stub.ENTRIES]
    assert res["mean_logprob"] == pytest.approx(sum(vals) / len(vals)) and res["min_logprob"] == min(vals)
    assert "logprobs" not in res
    stored = m.analysis.store.list(1)[0]["result"]
    assert stored["mean_logprob"] == res["mean_logprob"] and stored["min_logprob"] == res["min_logprob"]
    plain = json.loads(post("/api/v1/query", {"question": "why?"}).body)["result"]
    assert "mean_logprob" not in plain and "logprobs" not in be.calls[-1]
    r = post("/api/v1/analyze", {"type": "root_cause", "parameters": {"logprobs": True}})
    assert r.code == 200 and json.loads(r.body)["result"]["min_logprob"] == min(vals)
    assert post("/api/v1/query", {"question": "why?", "logprobs": True, "stream": True}).code == 400
    assert post("/api/v1/query", {"question": "why?", "logprobs": "yes"}).code == 400


def test_logprob_summary_of_an_empty_answer_is_null():
    from k8s_llm_monitor_amd.llm.service import logprob_summary

    assert logprob_summary([]) == {"mean_logprob": None, "min_logprob": None}
    assert logprob_summary(None) == {"mean_logprob": None, "min_logprob": None}


def test_openai_backend_forwards_logprobs_and_hands_the_content_back(monkeypatch):
    from k8s_llm_monitor_amd.llm import service

    sent = []
    content = [{"token": "ok", "logprob": -0.1, "bytes": [111, 107], "top_logprobs": []}]

    class _Resp:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def read(self):
            return json.dumps({"choices": [{"message": {"content": "ok"}, "logprobs": {"content": content}}]}).encode()

    monkeypatch.setattr(service.urllib.request, "urlopen",
                        lambda req, timeout=None: sent.append(json.loads(req.data)) or _Resp())
    be = service.OpenAIBackend("key", "http://upstream.invalid/v1", "m", 16, 0.1, 5.0)
    assert "logprobs" not in be.generate("q") and "logprobs" not in sent[0]
    g = be.generate("q", logprobs=True, top_logprobs=4)
    assert sent[1]["logprobs"] is True and sent[1]["top_logprobs"] == 4 and g["logprobs"] == content
    assert "logprobs" not in service.RuleBackend().generate("q", logprobs=True, top_logprobs=2)
