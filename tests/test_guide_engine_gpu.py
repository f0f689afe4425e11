"""Constrained decoding through the engine on the GPU (llama-tiny-d128, random weights): graphs
and pipelined decode with guided and unguided requests side by side, preemption by recompute,
chunked prefill, penalties and logprobs on top of a guide, and the stats."""
import json
import re

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.engine.guide import compile_guide

pytestmark = pytest.mark.gpu

CHOICE = {"choice": ["low", "medium", "high"]}
REGEX = {"regex": r"pod-[a-z]{3}-\d{2}"}
OBJ = {"json_schema": {"type": "object", "properties": {"severity": {"enum": ["low", "high"]},
                                                        "restarts": {"type": "integer"},
                                                        "ready": {"type": "boolean"}}}}
SPECS = [CHOICE, REGEX, OBJ, None]
PROMPTS = [f"pod default/api-{i} restarted {i * 3} times: what is the severity?" for i in range(64)]
# the batch whose greedy answers are compared between two engines: no 16-token block in common with
# PROMPTS, so the prefix cache gives both engines the same (empty) start
PLAIN = [f"{i} nodes of zone {chr(97 + i)} are NotReady since the last kubelet restart: why?" for i in range(16)]


def engine(**kw):
    ops.native()
    cfg = dict(model="llama-tiny-d128", max_num_seqs=64, max_model_len=1024, num_blocks=1024, seed=0)
    cfg.update(kw)
    eng = LLMEngine(EngineConfig(**cfg), device="cuda:0")
    eng.warmup()
    return eng


def run(eng, seqs):
    while eng.has_work():
        eng.step()
    torch.cuda.synchronize()
    return seqs


def check(eng, seq, spec):
    text = eng.decode_text(seq)
    assert seq.finish_reason == "stop", (spec, text, seq.finish_reason)
    assert compile_guide(spec).matches(text), (spec, text)
    if spec is CHOICE:
        assert text in CHOICE["choice"]
    elif spec is REGEX:
        assert re.fullmatch(REGEX["regex"], text)
    else:
        d = json.loads(text)
        assert list(d) == ["severity", "restarts", "ready"] and d["severity"] in ("low", "high") \
            and type(d["restarts"]) is int and type(d["ready"]) is bool


@pytest.fixture(scope="module")
def plain_greedy():
    """Greedy answers of an engine in which the feature was never enabled."""
    eng = engine()
    seqs = run(eng, [eng.add_request(p, SamplingParams(max_tokens=24, temperature=0.0)) for p in PLAIN])
    st = eng.stats()
    assert st["guide_enabled"] is False and st["guide_state_bytes"] == 0 and eng.runner.gd is None
    return [list(s.output_ids) for s in seqs]


def test_64_mixed_requests_and_unguided_rows_unchanged(plain_greedy):
    eng = engine()
    st = eng.stats()
    assert (st["guide_enabled"], st["guide_state_bytes"], st["guides_resident"], st["guide_slots_in_use"]) == \
        (False, 0, 0, 0)
    seqs, specs = [], []
    for i in range(64):
        spec = SPECS[i % 4]
        temp = 1.0 if (i // 4) % 2 == 0 else 0.0
        specs.append(spec)
        seqs.append(eng.add_request(PROMPTS[i], SamplingParams(max_tokens=24 if spec is None else 96,
                                                               temperature=temp, guide=spec)))
    st = eng.stats()
    assert st["guide_enabled"] and st["guides_resident"] == 3 and st["guide_state_bytes"] == eng.runner.gd.nbytes > 0
    assert eng.runner.gd.rows == 64 * 512
    used = 0
    while eng.has_work():
        eng.step()
        used = max(used, eng.stats()["guide_slots_in_use"])
    assert used == 48 and eng.stats()["guide_slots_in_use"] == 0 and eng.runner.gd.slots_in_use == 0
    assert eng.stats()["decode_steps"] > 0 and eng.runner.graphs
    for s, spec in zip(seqs, specs):
        if spec is not None:
            check(eng, s, spec)
    assert all(len(s.output_ids) > 0 for s, spec in zip(seqs, specs) if spec is None)
    # Unguided greedy answers, token for token those of an engine in which the feature was never
    # enabled: the same batch through the graphs captured with the guide state.  (The same batch,
    # because a prompt's first token depends on which prefill GEMM form its step's row count
    # picks; that unguided rows beside guided ones sample as without the feature is checked bit
    # for bit on the sampler itself, tests/test_guide_gpu.py.)
    again = run(eng, [eng.add_request(p, SamplingParams(max_tokens=24, temperature=0.0)) for p in PLAIN])
    assert [list(s.output_ids) for s in again] == plain_greedy


def test_preemption_by_recompute_keeps_full_matches():
    eng = engine(max_num_seqs=8, num_blocks=14, max_model_len=256)
    long_re = {"regex": r"[a-z]{60}-\d{20}"}
    specs = [long_re, OBJ, long_re, REGEX, long_re, CHOICE]
    seqs = [eng.add_request(PROMPTS[i][:40], SamplingParams(max_tokens=200, temperature=1.0, guide=s))
            for i, s in enumerate(specs)]
    run(eng, seqs)
    assert eng.stats()["preemptions"] > 0
    for s, spec in zip(seqs, specs):
        text = eng.decode_text(s)
        assert s.finish_reason == "stop" and compile_guide(spec).matches(text), (spec, text, s.n_preemptions)
    assert any(s.n_preemptions > 0 and len(s.output_ids) > 8 for s in seqs)


def test_chunked_prefill_does_not_advance_on_intermediate_chunks():
    eng = engine(max_num_seqs=4, max_prefill_tokens=32, mixed_prefill_tokens=32)
    prompt = " ".join(PROMPTS[:12])
    assert len(eng.tokenizer.encode(prompt)) > 3 * 32
    seqs = [eng.add_request(prompt, SamplingParams(max_tokens=40, temperature=1.0, guide=REGEX)),
            eng.add_request(PROMPTS[1], SamplingParams(max_tokens=40, temperature=0.0, guide=CHOICE))]
    gd = eng.runner.gd
    rows = gd.resident_rows(compile_guide(REGEX))
    seen_mid_chunk = False
    while eng.has_work():
        eng.step()
        s = seqs[0]
        slot = eng.runner._gd_slot.get(s.seq_id)
        if slot is not None and 0 < s.num_computed < len(s.prompt_ids) and not s.output_ids:
            torch.cuda.synchronize()
            assert int(gd.state[slot]) == int(rows[0])  # still the start state
            seen_mid_chunk = True
    assert seen_mid_chunk
    check(eng, seqs[0], REGEX)
    check(eng, seqs[1], CHOICE)


def test_penalties_and_logprobs_with_a_guide():
    eng = engine(max_num_seqs=8)
    p = SamplingParams(max_tokens=96, temperature=1.0, guide=OBJ, repetition_penalty=2.0, presence_penalty=0.5,
                       frequency_penalty=0.25, logprobs=True, top_logprobs=3)
    q = SamplingParams(max_tokens=96, temperature=0.0, guide=REGEX, logprobs=True, top_logprobs=2)
    seqs = run(eng, [eng.add_request(PROMPTS[0], p), eng.add_request(PROMPTS[1], q),
                     eng.add_request(PROMPTS[2], SamplingParams(max_tokens=8, temperature=0.0))])
    check(eng, seqs[0], OBJ)
    check(eng, seqs[1], REGEX)
    for s, n_top in ((seqs[0], 3), (seqs[1], 2)):
        assert len(s.output_logprobs) == len(s.output_ids)
        forced = 0
        for tok, (lp, top) in zip(s.output_ids, s.output_logprobs):
            assert lp <= 0.0 and len(top) == n_top and top[0][1] >= lp - 1e-6
            forced += top[0][0] != tok
        # the logprobs are those of the unconstrained distribution: a random model's favourite token
        # is rarely the one the guide allows
        assert forced > 0
    st = eng.stats()
    assert st["penalty_slots_in_use"] == 0 and st["guide_slots_in_use"] == 0 and st["logprobs_enabled"]
