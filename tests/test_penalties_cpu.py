"""Sampling penalties without a GPU: the reference definition, the CPU-resident state, the CPU
engine (slots, preemption, a neutral neighbour) and the public surface (config, chat route)."""
import json
import types

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.models import AttnMeta
from k8s_llm_monitor_amd.ops import reference as ref


# ---------------------------------------------------------------- the definition

def test_apply_penalties_matches_a_per_element_loop():
    #          count 0     prompt only   output only   both          count 0 (negative)
    logits = [1.5, -2.0,   3.0, -1.25,   0.75, -4.0,   2.5, -0.5,    0.0, -3.0]
    seen = [0, 0,          1, 1,         0, 0,         1, 1,         0, 0]
    count = [0, 0,         0, 0,         1, 3,         2, 5,         0, 0]
    rep, presence, frequency = 1.3, 0.4, 0.25
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731 - every step rounded to fp32
    inv_rep = f32(1.0 / rep)
    want = []
    for x, s, c in zip(logits, seen, count):
        x = f32(x)
        if s or c > 0:
            x = x * inv_rep if x > 0 else x * f32(rep)
        x = x - f32(frequency) * f32(float(c))
        x = x - f32(presence) * f32(1.0 if c > 0 else 0.0)
        want.append(float(x))
    got = ref.apply_penalties(torch.tensor(logits), torch.tensor(seen, dtype=torch.bool), torch.tensor(count),
                              rep, presence, frequency)
    assert got.dtype == torch.float32
    assert got.tolist() == want
    # untouched entries are returned as they were; neutral penalties change nothing at all
    assert got[0] == 1.5 and got[1] == -2.0 and got[8] == 0.0 and got[9] == -3.0
    same = ref.apply_penalties(torch.tensor(logits), torch.tensor(seen, dtype=torch.bool), torch.tensor(count),
                               1.0, 0.0, 0.0)
    assert same.tolist() == logits
    assert ref.penalty_inv_rep(rep) == float(inv_rep)


# ---------------------------------------------------------------- the CPU-resident state

def test_sampling_params_defaults_are_neutral_and_appended():
    p = SamplingParams()
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty) == (1.0, 0.0, 0.0)
    assert not p.has_penalties()
    assert SamplingParams(frequency_penalty=0.5).has_penalties()
    # positional construction keeps its meaning (engine.py rebuilds params from a tuple)
    q = SamplingParams(7, 0.5, 3, 0.9, True, (1,), 1.2, 0.3, 0.4)
    assert (q.max_tokens, q.temperature, q.top_k, q.top_p, q.ignore_eos, q.stop_token_ids) == (7, 0.5, 3, 0.9, True, (1,))
    assert (q.repetition_penalty, q.presence_penalty, q.frequency_penalty) == (1.2, 0.3, 0.4)


def test_reset_then_cpu_sample_counts_one_token_per_row_with_a_slot():
    V, B = 37, 4
    st = ops.PenaltyState(3, V, "cpu")
    st.reset(2, [1, 5, 5, 9], [5, 7, 7, 7], rep=2.0, presence=0.5, frequency=0.25)
    st.reset(0, [3], [], frequency=4.0)
    assert st.counts()[2].nonzero().flatten().tolist() == [5, 7]
    assert int(st.counts()[2, 5]) == 1 and int(st.counts()[2, 7]) == 3
    assert st.seen()[2].nonzero().flatten().tolist() == [1, 5, 9]
    assert st.seen()[0].nonzero().flatten().tolist() == [3] and int(st.counts()[0].sum()) == 0
    assert int(st.counts()[1].sum()) == 0 and not bool(st.seen()[1].any())
    g = torch.Generator().manual_seed(0)
    logits = (torch.randint(-128, 129, (B, V), generator=g).float() / 16)
    logits[1, 7] = 8.5  # slot 2's most counted token would win its row without penalties
    slots = torch.tensor([-1, 2, 0, -1], dtype=torch.int32)
    before_c, before_s = st.counts().clone(), st.seen().clone()
    toks = ops.sample(logits, penalties=st, slots=slots)
    want = [int(logits[0].argmax()),
            int(ref.apply_penalties(logits[1], before_s[2], before_c[2], 2.0, 0.5, 0.25).argmax()),
            int(ref.apply_penalties(logits[2], before_s[0], before_c[0], 1.0, 0.0, 4.0).argmax()),
            int(logits[3].argmax())]
    assert toks.tolist() == want and want[1] != 7
    delta = st.counts() - before_c
    assert int(delta.sum()) == 2 and int(delta[2, want[1]]) == 1 and int(delta[0, want[2]]) == 1
    assert torch.equal(st.seen(), before_s)
    # the same call without the state is the sampler as it was
    assert ops.sample(logits).tolist() == [int(r.argmax()) for r in logits]
    with pytest.raises(ValueError):
        ops.sample(logits, penalties=st)  # a state needs the rows' slots


def test_count_saturates_at_its_storage_maximum():
    V = 16
    st = ops.PenaltyState(1, V, "cpu")
    st.reset(0, [4], [], frequency=-1.0)  # a negative frequency penalty: the counted token keeps winning
    st.table[0, 4] = st.table[0, 4] | ops.PenaltyState.MAX_COUNT
    assert int(st.counts()[0, 4]) == ops.PenaltyState.MAX_COUNT and bool(st.seen()[0, 4])
    logits = torch.zeros(1, V)
    for _ in range(2):
        assert ops.sample(logits, penalties=st, slots=torch.zeros(1, dtype=torch.int32)).tolist() == [4]
    assert int(st.counts()[0, 4]) == ops.PenaltyState.MAX_COUNT and bool(st.seen()[0, 4])
    assert int(st.counts()[0].sum()) == ops.PenaltyState.MAX_COUNT
    # reset saturates too
    st.reset(0, [], [2] * (ops.PenaltyState.MAX_COUNT + 10))
    assert int(st.counts()[0, 2]) == ops.PenaltyState.MAX_COUNT and not bool(st.seen()[0].any())


# ---------------------------------------------------------------- the CPU engine

STEPS = 48
PEN = SamplingParams(max_tokens=STEPS, temperature=0.0, ignore_eos=True, frequency_penalty=1000.0)
NEUTRAL = SamplingParams(max_tokens=STEPS, temperature=0.0, ignore_eos=True)


def _engine(**kw):
    cfg = dict(model="llama-tiny", max_num_seqs=4, max_model_len=256, num_blocks=64, use_graphs=False,
               dtype="float32")
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


def _last_logits(model, ids):
    n = len(ids)
    meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32),
                    slot_mapping=torch.full((n,), -1, dtype=torch.int32),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32), logits_idx=torch.tensor([n - 1]))
    return model.forward(torch.tensor(ids, dtype=torch.int32), meta, None)[0].float()


def _run(eng, reqs):
    seqs = [eng.add_request(p, sp) for p, sp in reqs]
    while eng.has_work():
        eng.step()
    return seqs


def test_cpu_engine_frequency_penalty_gives_distinct_tokens_and_leaves_the_neighbour_alone():
    eng = _engine()
    assert eng.stats()["penalty_state_bytes"] == 0 and eng.runner.memory_report()["penalty_state_bytes"] == 0
    solo = _run(eng, [("node-003 NotReady 为什么", NEUTRAL)])[0]
    assert eng.stats()["penalty_state_bytes"] == 0  # nothing is allocated for neutral requests
    pen, neutral = _run(eng, [("pod crashloop in kube-system", PEN), ("node-003 NotReady 为什么", NEUTRAL)])
    assert len(pen.output_ids) == STEPS and len(set(pen.output_ids)) == STEPS
    assert neutral.output_ids == solo.output_ids
    assert len(set(solo.output_ids)) < STEPS  # the near-greedy loop the penalty is there to break
    st = eng.stats()
    assert st["penalty_state_bytes"] == eng.runner.pen.nbytes > 0 and st["penalty_slots_in_use"] == 0
    # the same tokens from a hand-rolled loop over the same model
    V = eng.model_cfg.vocab_size
    seen = torch.zeros(V, dtype=torch.bool)
    seen[pen.prompt_ids] = True
    count = torch.zeros(V, dtype=torch.int64)
    ids, want = list(pen.prompt_ids), []
    for _ in range(STEPS):
        x = ref.apply_penalties(_last_logits(eng.model, ids), seen, count, 1.0, 0.0, 1000.0)
        t = int(x.argmax())
        want.append(t)
        count[t] += 1
        ids.append(t)
    assert pen.output_ids == want


def test_cpu_engine_penalty_survives_preemption():
    eng = _engine(max_num_seqs=8, num_blocks=12)
    seqs = _run(eng, [("a" * 30, PEN)] * 6)
    assert sum(s.n_preemptions for s in seqs) > 0 and eng.counters["preemptions"] > 0
    for s in seqs:
        assert len(s.output_ids) == STEPS and len(set(s.output_ids)) == STEPS
    assert seqs[0].output_ids == seqs[-1].output_ids  # the recompute rebuilt the same counts
    assert eng.stats()["penalty_slots_in_use"] == 0 and eng.blocks.num_free == 12


def test_cpu_engine_slot_is_released_on_abort_and_repetition_penalty_validated():
    eng = _engine()
    s = eng.add_request("pod crashloop", PEN)
    eng.step()
    assert eng.stats()["penalty_slots_in_use"] == 1
    eng.abort(s)
    assert eng.stats()["penalty_slots_in_use"] == 0
    with pytest.raises(ValueError):
        eng.add_request("x", SamplingParams(repetition_penalty=0.0))


def test_engine_refuses_penalties_with_tensor_parallelism():
    eng = _engine()
    eng.ps = types.SimpleNamespace(tp_size=2, tp_rank=0)
    with pytest.raises(ValueError, match="tensor parallelism"):
        eng.add_request("x", PEN)
    eng.add_request("x", NEUTRAL)  # neutral requests are not affected


# ---------------------------------------------------------------- config and the chat route

def test_config_keys_reach_the_backends():
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend, OpenAIBackend
    from k8s_llm_monitor_amd.monitor.app import make_llm_backend
    from k8s_llm_monitor_amd.monitor.config import from_dict

    d = from_dict({}).llm
    assert (d.repetition_penalty, d.presence_penalty, d.frequency_penalty) == (1.0, 0.0, 0.0)
    cfg = from_dict({"llm": {"provider": "openai", "api_key": "k", "repetition_penalty": 1.1,
                             "presence_penalty": 0.5, "frequency_penalty": "0.25"}})
    assert (cfg.llm.repetition_penalty, cfg.llm.presence_penalty, cfg.llm.frequency_penalty) == (1.1, 0.5, 0.25)
    be = make_llm_backend(cfg)[0]
    assert isinstance(be, OpenAIBackend) and (be.presence_penalty, be.frequency_penalty) == (0.5, 0.25)

    eng = _engine()
    got = []
    svc = types.SimpleNamespace(engine=eng, submit=lambda prompt, p, rid, deadline=None: got.append(p) or _Done(eng))
    lb = LocalEngineBackend(svc, max_tokens=8, repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)
    lb.generate("q")
    lb.generate("q", presence_penalty=-1.0, repetition_penalty=2.0)
    assert (got[0].repetition_penalty, got[0].presence_penalty, got[0].frequency_penalty) == (1.1, 0.5, 0.25)
    assert (got[1].repetition_penalty, got[1].presence_penalty, got[1].frequency_penalty) == (2.0, -1.0, 0.25)


class _Done:
    """A finished future of the engine service."""

    def __init__(self, eng):
        from k8s_llm_monitor_amd.engine.sequence import Sequence

        self.seq = Sequence(prompt_ids=[1], params=SamplingParams(), output_ids=[2], finish_reason="length")

    def result(self, timeout=None):
        return "text", self.seq


def test_openai_backend_forwards_the_two_openai_fields(monkeypatch):
    from k8s_llm_monitor_amd.llm import service

    sent = []

    class _Resp:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def read(self):
            return json.dumps({"choices": [{"message": {"content": "ok"}}]}).encode()

    monkeypatch.setattr(service.urllib.request, "urlopen",
                        lambda req, timeout=None: sent.append(json.loads(req.data)) or _Resp())
    be = service.OpenAIBackend("key", "http://upstream.invalid/v1", "m", 16, 0.1, 5.0)
    be.generate("q")
    be.generate("q", presence_penalty=0.5, frequency_penalty=-0.25, repetition_penalty=1.2)
    assert "presence_penalty" not in sent[0] and "frequency_penalty" not in sent[0]
    assert sent[1]["presence_penalty"] == 0.5 and sent[1]["frequency_penalty"] == -0.25
    assert "repetition_penalty" not in sent[1]


def _monitor(backend):
    from k8s_llm_monitor_amd.monitor.app import build_monitor
    from k8s_llm_monitor_amd.monitor.cluster.fake import FakeCluster
    from k8s_llm_monitor_amd.monitor.config import from_dict

    m = build_monitor(from_dict({"llm": {"provider": "none"}}), backend=FakeCluster.build(seed=2),
                      start_manager=False, llm=True)
    m.analysis.backend = backend
    return m.app


class _Recorder:
    provider, model = "stub", "stub"

    def __init__(self):
        self.calls = []

    def count_tokens(self, text):
        return len(text)

    def generate(self, prompt, **kw):
        from k8s_llm_monitor_amd.llm.service import GenResult

        self.calls.append(kw)
        return GenResult(text="ok", model="stub", provider="stub", prompt_tokens=1, completion_tokens=1,
                         latency_ms=0.0, ttft_ms=0.0, finish_reason="stop")


def _chat(app, **fields):
    body = {"messages": [{"role": "user", "content": "hi"}], **fields}
    return app.handle("POST", "/v1/chat/completions", json.dumps(body).encode())


def test_chat_route_passes_valid_penalties_and_refuses_invalid_ones():
    be = _Recorder()
    app = _monitor(be)
    assert _chat(app).code == 200
    assert not {"presence_penalty", "frequency_penalty", "repetition_penalty"} & set(be.calls[-1])
    assert _chat(app, presence_penalty=2, frequency_penalty=-2.0, repetition_penalty=1.3).code == 200
    kw = be.calls[-1]
    assert (kw["presence_penalty"], kw["frequency_penalty"], kw["repetition_penalty"]) == (2.0, -2.0, 1.3)
    assert _chat(app, repetition_penalty=10).code == 200
    n = len(be.calls)
    for bad in ({"presence_penalty": 2.5}, {"presence_penalty": "1"}, {"frequency_penalty": -2.01},
                {"frequency_penalty": True}, {"repetition_penalty": 0}, {"repetition_penalty": -1},
                {"repetition_penalty": 10.5}, {"repetition_penalty": [1]}):
        assert _chat(app, **bad).code == 400, bad
    assert len(be.calls) == n  # nothing invalid reached the backend


def test_chat_route_answers_400_when_the_engine_cannot_apply_penalties():
    from k8s_llm_monitor_amd.engine import EngineService
    from k8s_llm_monitor_amd.llm.service import LocalEngineBackend

    eng = _engine()
    eng.ps = types.SimpleNamespace(tp_size=2, tp_rank=0)  # as a TP leader sees itself
    svc = EngineService(eng)
    try:
        app = _monitor(LocalEngineBackend(svc, max_tokens=4, temperature=0.0, timeout_s=60.0))
        r = _chat(app, frequency_penalty=0.5, max_tokens=4)
        assert r.code == 400 and b"tensor parallelism" in r.body
        assert _chat(app, max_tokens=4).code == 200
    finally:
        svc.close()
