"""Sampling penalties on the GPU: the penalising sampler against ``ref.apply_penalties`` (bit for
bit: every input is chosen so that fp32 penalisation is exact), the device-resident state (update,
reset, saturation), a captured step that keeps its own counts, and the engine with graphs and
pipelined decode.

Exactness: logits are multiples of 1/16 in [-8, 8] (exact in bf16), rep is 1, 2 or 4, presence and
frequency are multiples of 1/8 and counts stay <= 64, so every product and difference is a small
multiple of 1/64 - exact in fp32 whatever the compiler contracts."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 50257), (5, 128256), (128, 32000)]


class Case:
    """B rows over V entries: bf16 logits in a view whose stride is not V, every sampler path
    among the rows, some rows without a slot, the others on shuffled slots of a state reset from
    known prompt / output ids, and the fp32 logits penalised by the reference."""

    def __init__(self, B, V, seed):
        ops.native()
        g = torch.Generator().manual_seed(seed)
        stride = (V + 7) // 8 * 8 + 8
        x = torch.randint(-128, 129, (B, V), generator=g).float() / 16  # many ties at every value
        buf = torch.zeros(B, stride, dtype=torch.bfloat16)
        buf[:, :V] = x.to(torch.bfloat16)
        assert torch.equal(buf[:, :V].float(), x)
        self.B, self.V, self.x = B, V, x
        self.logits = buf.to(DEV)[:, :V]
        assert self.logits.stride(0) != V
        # rows: greedy, sampled, top-k, top-p, top-k + top-p (the last three take the whole-row path)
        kinds = [(0.0, 0, 1.0), (0.75, 0, 1.0), (1.0, 40, 1.0), (0.5, 0, 0.8), (1.25, 64, 0.9)]
        rows = [kinds[b % len(kinds)] for b in range(B)]
        self.temps = torch.tensor([r[0] for r in rows], device=DEV)
        self.top_k = torch.tensor([r[1] for r in rows], device=DEV, dtype=torch.int32)
        self.top_p = torch.tensor([r[2] for r in rows], device=DEV)
        self.rng = torch.tensor([1234 + seed, 17], device=DEV, dtype=torch.int64)
        n_slots = B + 3
        perm = torch.randperm(n_slots, generator=g)[:B].tolist()
        self.slots = [-1 if b % 4 == 2 else perm[b] for b in range(B)]  # every path also without a slot
        if B >= 10:
            self.slots[0:10:5] = [-1, -1]  # ... and greedy rows of both kinds in a large batch
        self.d_slots = torch.tensor(self.slots, device=DEV, dtype=torch.int32)
        self.state = ops.PenaltyState(n_slots, V, DEV)
        self.plain = ops.sample(self.logits, self.temps, self.top_k, self.top_p, self.rng.clone())  # no penalties
        self.decided = []  # greedy rows whose unpenalised winner is penalised below the rest of its row
        self.resets = {}
        pre = x.clone()
        for b, slot in enumerate(self.slots):
            if slot < 0:
                continue
            # the row's best tokens are the ones penalised, so the penalties decide the answer
            top = torch.topk(x[b], 300).indices
            prompt = torch.cat([top[torch.randint(0, 300, (40,), generator=g)],
                                torch.randint(0, V, (160,), generator=g)]).tolist()
            output = top[torch.randint(0, 150, (200,), generator=g)].tolist()
            output += [int(self.plain[b])] * int(torch.randint(1, 40, (1,), generator=g))
            rep = [1.0, 2.0, 4.0][int(torch.randint(0, 3, (1,), generator=g))]
            presence = int(torch.randint(-8, 17, (1,), generator=g)) / 8
            frequency = int(torch.randint(-4, 17, (1,), generator=g)) / 8
            if rows[b][0] == 0.0:  # a greedy row: its winner (generated before) loses at least 1/8
                presence, frequency = abs(presence), abs(frequency) + 0.125
                self.decided.append(b)
            self.resets[slot] = (prompt, output, rep, presence, frequency)
            self.state.reset(slot, prompt, output, rep, presence, frequency)
            seen = torch.zeros(V, dtype=torch.bool)
            seen[prompt] = True
            count = torch.bincount(torch.tensor(output), minlength=V)
            assert int(count.max()) <= 64
            pre[b] = ref.apply_penalties(x[b], seen, count, rep, presence, frequency)
        self.pre = pre.to(DEV)  # fp32, contiguous: what today's sampler is given

    def sample(self, **kw):
        return ops.sample(self.logits, self.temps, self.top_k, self.top_p, self.rng.clone(), **kw)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"B{s[0]}-V{s[1]}")
def case(request):
    B, V = request.param
    return Case(B, V, seed=B)


def test_penalised_sampler_equals_reference_then_counts_its_tokens(case):
    st = case.state
    before = st.table.clone()
    want = ops.sample(case.pre, case.temps, case.top_k, case.top_p, case.rng.clone())
    got = case.sample(penalties=st, slots=case.d_slots)
    assert torch.equal(got, want)
    plain = case.sample()
    has = torch.tensor([s >= 0 for s in case.slots], device=DEV)
    assert torch.equal(plain, case.plain) and torch.equal(plain[~has], got[~has])  # no slot: the sampler as it was
    assert case.decided and all(int(got[b]) != int(plain[b]) for b in case.decided)  # the penalties decide tokens
    # the state: +1 at (slot, token) of every row with a slot, nothing else, seen bits untouched
    delta = (st.table.to(torch.int32) - before.to(torch.int32)).cpu()
    expect = torch.zeros_like(delta)
    for b, slot in enumerate(case.slots):
        if slot >= 0:
            expect[slot, int(got[b])] += 1
    assert torch.equal(delta, expect)
    assert torch.equal(st.table < 0, before < 0)
    st.table.copy_(before)  # the case is shared: leave it as it was


def test_reset_gives_exact_counts_and_seen_bits(case):
    st, V = case.state, case.V
    counts, seen = st.counts().cpu(), st.seen().cpu()
    assert counts.shape == (st.slots, V) and seen.shape == (st.slots, V)
    for slot in range(st.slots):
        prompt, output, rep, presence, frequency = case.resets.get(slot, ([], [], 1.0, 0.0, 0.0))
        want_seen = torch.zeros(V, dtype=torch.bool)
        want_seen[torch.tensor(prompt, dtype=torch.long)] = True
        assert torch.equal(seen[slot], want_seen)
        assert torch.equal(counts[slot].long(), torch.bincount(torch.tensor(output, dtype=torch.long), minlength=V))
        assert st.params[slot].tolist() == [rep, ref.penalty_inv_rep(rep), presence, frequency]
    assert int(st.table[:, V:].abs().sum()) == 0  # the padding of a row stays clear


def test_reset_of_one_slot_leaves_the_others_alone():
    V = 50257
    st = ops.PenaltyState(4, V, DEV)
    for slot in range(4):
        st.reset(slot, [slot, 7, V - 1], [slot + 10] * (slot + 1), rep=2.0, presence=0.5, frequency=0.25)
    before = st.table.clone(), st.params.clone()
    ids = [3, 3, 3, V - 1, 0, 3, V - 1, 9]
    st.reset(2, [5, 5, V - 2, 9, V + 3, -1], ids + [V, -7], rep=4.0, presence=-0.125, frequency=1.5)  # ids outside [0, V) are skipped
    others = [0, 1, 3]
    assert torch.equal(st.table[others], before[0][others]) and torch.equal(st.params[others], before[1][others])
    c, s = st.counts()[2].cpu(), st.seen()[2].cpu()
    assert torch.equal(c.long(), torch.bincount(torch.tensor(ids), minlength=V))
    assert s.nonzero().flatten().tolist() == [5, 9, V - 2]
    assert st.params[2].tolist() == [4.0, 0.25, -0.125, 1.5]
    assert int(st.table[:, V:].abs().sum()) == 0


def test_counts_saturate():
    V, M = 8192, ops.PenaltyState.MAX_COUNT
    st = ops.PenaltyState(2, V, DEV)
    st.reset(1, [5], [5] * (M + 100) + [6] * 3, frequency=-1.0)
    assert int(st.counts()[1, 5]) == M and int(st.counts()[1, 6]) == 3 and bool(st.seen()[1, 5])
    assert int(st.counts()[1].sum()) == M + 3
    # a negative frequency penalty keeps token 5 winning: its count stays at the maximum
    logits = torch.zeros(1, V, device=DEV, dtype=torch.bfloat16)
    slots = torch.ones(1, device=DEV, dtype=torch.int32)
    for _ in range(2):
        assert ops.sample(logits, penalties=st, slots=slots).tolist() == [5]
    assert int(st.counts()[1, 5]) == M and bool(st.seen()[1, 5]) and int(st.counts()[1].sum()) == M + 3
    assert int(st.counts()[0].sum()) == 0


def test_captured_step_keeps_its_own_counts():
    B, V = 2, 32000
    g = torch.Generator().manual_seed(5)
    x = -torch.randint(0, 129, (B, V), generator=g).float() / 16  # everything else is <= 0
    ranked = [[31999, 17, 4096, 12345, 8, 20000], [3, 31000, 77, 15000, 9000, 1]]
    for b in range(B):
        x[b, ranked[b]] = torch.arange(8.0, 2.0, -1.0)  # top values 1 apart
    logits = x.to(torch.bfloat16).to(DEV)
    st = ops.PenaltyState(B, V, DEV)
    rng = torch.tensor([9, 0], device=DEV, dtype=torch.int64)
    d_pslot = torch.tensor([0, 1], device=DEV, dtype=torch.int32)
    out = torch.zeros(B, device=DEV, dtype=torch.int32)

    def step():
        ops.sample(logits, None, None, None, rng, out=out, advance=True, penalties=st, slots=d_pslot)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for b in range(B):
        st.reset(b, [], [], frequency=8.0)  # drop what the warm-up counted
    rng[1] = 0
    got = []
    for i in range(4):
        if i == 2:
            d_pslot.copy_(torch.tensor([0, -1], dtype=torch.int32))  # row 1 loses its penalties, no recapture
        graph.replay()
        got.append(out.tolist())
    assert [t[0] for t in got] == ranked[0][:4]
    assert [t[1] for t in got] == ranked[1][:2] + [ranked[1][0]] * 2
    assert int(rng[1]) == 4
    c = st.counts().cpu()
    assert int(c[0].sum()) == 4 and all(int(c[0, t]) == 1 for t in ranked[0][:4])
    assert int(c[1].sum()) == 2 and all(int(c[1, t]) == 1 for t in ranked[1][:2])


# ---------------------------------------------------------------- the engine

STEPS = 48
PEN = SamplingParams(max_tokens=STEPS, temperature=0.0, ignore_eos=True, frequency_penalty=1000.0)
NEUTRAL = SamplingParams(max_tokens=STEPS, temperature=0.0, ignore_eos=True)


def _run(eng, reqs):
    seqs = [eng.add_request(p, sp) for p, sp in reqs]
    while eng.has_work():
        eng.step()
    return seqs


@pytest.fixture(scope="module")
def engine():
    eng = LLMEngine(EngineConfig(model="llama-tiny-d128", max_num_seqs=8, max_model_len=1024, num_blocks=256,
                                 seed=0), device=DEV)
    eng.warmup()
    assert eng.runner.graphs and eng.cfg.pipeline
    return eng


def test_engine_allocates_lazily_and_penalises_one_row_of_the_batch(engine):
    eng = engine
    assert eng.stats()["penalty_state_bytes"] == 0 and eng.runner.pen is None
    solo = _run(eng, [("node-003 NotReady 为什么", NEUTRAL)])[0]
    assert eng.stats()["penalty_state_bytes"] == 0
    buckets = sorted(eng.runner.graphs)
    pen, neutral = _run(eng, [("pod crashloop in kube-system", PEN), ("node-003 NotReady 为什么", NEUTRAL)])
    assert len(pen.output_ids) == STEPS and len(set(pen.output_ids)) == STEPS
    assert neutral.output_ids == solo.output_ids
    st = eng.stats()
    V = eng.model_cfg.vocab_size
    assert st["penalty_state_bytes"] == 8 * V * 2 + 8 * 16 and st["penalty_slots_in_use"] == 0
    assert eng.runner.memory_report()["penalty_state_bytes"] == st["penalty_state_bytes"]
    assert sorted(eng.runner.graphs) == buckets  # the decode steps are still replayed


def test_engine_releases_the_slot_of_a_cancelled_request(engine):
    eng = engine
    a = eng.add_request("pod crashloop in kube-system", PEN)
    b = eng.add_request("why is pod default/api not ready?", PEN)
    for _ in range(5):
        eng.step()
    assert eng.stats()["penalty_slots_in_use"] == 2
    eng.abort(a)
    assert eng.stats()["penalty_slots_in_use"] == 1
    while eng.has_work():
        eng.step()
    assert eng.stats()["penalty_slots_in_use"] == 0
    assert len(b.output_ids) == STEPS and len(set(b.output_ids)) == STEPS


def test_engine_penalty_survives_preemption():
    eng = LLMEngine(EngineConfig(model="llama-tiny-d128", max_num_seqs=8, max_model_len=256, num_blocks=12, seed=0),
                    device=DEV)
    eng.warmup()
    seqs = _run(eng, [("a" * 30, PEN)] * 6)
    assert sum(s.n_preemptions for s in seqs) > 0
    for s in seqs:
        assert len(s.output_ids) == STEPS and len(set(s.output_ids)) == STEPS
    assert eng.stats()["penalty_slots_in_use"] == 0
