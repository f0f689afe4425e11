"""Constrained decoding on the GPU: the mask-build kernel bit for bit against ``ref.guide_mask``,
the guided sampler token for token against the same launch over logits whose disallowed entries
were set to -inf beforehand (same ``rng``), and the device-resident state against the host walk
(``ref.guide_advance``) - per launch, over replays of a captured graph, on an eos draw and after a
reset.

Logits are multiples of 1/16 in [-8, 8] (exact in bf16), so the bf16 and the fp32 launches read the
same numbers; penalties use rep in {1, 2, 4} and multiples of 1/8, exact in fp32."""
import random

import numpy as np
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine.guide import compile_guide
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIMIT = 512
ALPHA = "abc019-{}\":,x"  # what the guides below are written over ("Q" is kept out of every random token)
EOS = (2, 300)


def make_vocab(V, seed=0):
    """256 single-byte tokens (bos / eos without bytes), random words over ALPHA, a few tokens
    without bytes (one of them the last id), a 40-byte and a 17-byte token."""
    r = random.Random(seed)
    vb = [bytes([i]) for i in range(256)]
    while len(vb) < V:
        vb.append("".join(r.choice(ALPHA) for _ in range(r.randint(1, 6))).encode())
    vb[1] = vb[2] = b""
    for t in EOS:
        vb[t] = b""
    for t in (257, 399, V - 1):
        vb[t] = b""  # ... also in the last, partial word of the mask
    vb[400] = b"a" * 40  # longer than the kernel keeps in registers
    vb[401] = b"abcabcabcabcabcab" + b"c"  # 17 bytes: one past the registers
    return vb


GUIDES = {
    1: {"regex": "a*"},
    2: {"regex": "a+"},
    33: {"regex": "[abc]{32}"},
    LIMIT: {"regex": "[ab]{%d}" % (LIMIT - 1)},
}


def guide(n):
    g = compile_guide(GUIDES[n], LIMIT)
    assert g.n == n
    return g


_expect = {}


def expect_mask(g, V):
    """The reference mask of a guide over ``make_vocab(V)``: computed once, shared, never written."""
    key = (g.key, V)
    if key not in _expect:
        _expect[key] = ref.guide_mask(g.trans, g.accept, make_vocab(V), EOS)
    return _expect[key]


def raw_bits(gs, rows):
    w = gs.mask[torch.as_tensor(np.asarray(rows)).to(DEV)].cpu().numpy().view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)


def check_rows(gs, g, rows, V):
    exp = expect_mask(g, V).numpy()
    bits = raw_bits(gs, rows)
    assert bits.shape[1] == gs.W * 32 and gs.W % 4 == 0
    assert np.array_equal(bits[:, :V], exp)
    assert not bits[:, V:].any()  # the padding of the last words
    assert np.array_equal(gs.popc[torch.as_tensor(np.asarray(rows)).to(DEV)].cpu().numpy(), exp.sum(1))
    assert torch.equal(gs.mask_bits(rows), torch.from_numpy(exp))


@pytest.mark.parametrize("V", [515, 1000, 1024, 32776])
@pytest.mark.parametrize("n", [1, 2, 33, LIMIT])
def test_mask_build_matches_reference(V, n):
    ops.native()
    g = guide(n)
    gs = ops.GuideState(4, V, make_vocab(V), EOS, DEV, rows=n + 5)
    rows = gs.load(g)
    assert len(rows) == n and len(set(rows.tolist())) == n
    check_rows(gs, g, rows, V)
    exp = expect_mask(g, V)
    assert not exp[:, [1, 257, 399, V - 1]].any()  # tokens without bytes
    assert torch.equal(exp[:, EOS[0]], torch.tensor(g.accept)) and torch.equal(exp[:, EOS[1]], exp[:, EOS[0]])
    assert bool(exp[0, 400]) == (n in (1, 2, LIMIT)) and bool(exp[0, 401]) == (n == 33)


def test_two_guides_interleaved_rows_and_eviction():
    ops.native()
    V = 1000
    g1, g2, g3 = guide(33), compile_guide({"choice": ["abc", "ab-0", "x"]}, LIMIT), guide(2)
    gs = ops.GuideState(4, V, make_vocab(V), EOS, DEV, rows=g1.n + g2.n)
    r = random.Random(3)
    r.shuffle(gs.free_rows)
    r1 = gs.load(g1)
    r.shuffle(gs.free_rows)
    r2 = gs.load(g2)
    assert min(r1) < max(r2) and min(r2) < max(r1)  # interleaved, not two blocks
    assert not set(r1.tolist()) & set(r2.tolist())
    check_rows(gs, g1, r1, V)
    check_rows(gs, g2, r2, V)
    assert gs.load(g1) is r1 and gs.guides_resident == 2
    # a slot holds g2; g3 needs rows: the unreferenced g1 goes, g2 stays as it was
    gs.reset(0, g2, [])
    r3 = gs.load(g3)
    assert gs.resident_rows(g1) is None and set(r3.tolist()) <= set(r1.tolist())
    check_rows(gs, g3, r3, V)
    check_rows(gs, g2, r2, V)
    with pytest.raises(RuntimeError):
        gs.load(compile_guide({"regex": "[abc]{60}"}, LIMIT))  # more rows than eviction can free
    gs.release(0)
    r1b = gs.load(g1)  # a second build after the eviction (g2 and g3 make room)
    check_rows(gs, g1, r1b, V)


def test_empty_row_is_refused():
    ops.native()
    vb = make_vocab(515)
    vb[ord("Q")] = b""  # no token spells "Q"
    gs = ops.GuideState(2, 515, vb, EOS, DEV, rows=16)
    with pytest.raises(ValueError):
        gs.load(compile_guide({"choice": ["Q"]}, LIMIT))
    assert len(gs.free_rows) == 16 and gs.guides_resident == 0


# ------------------------------------------------------------------------------------------ sampler

KINDS = [(0.0, 0, 1.0), (0.75, 0, 1.0), (1.0, 40, 1.0), (0.5, 0, 0.8), (1.25, 64, 0.9)]
SPECS = [{"regex": "[abc]{32}"}, {"choice": ["abc", "ab-0", "x"]},
         {"json_schema": {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"enum": ["x", "c"]}}}},
         {"regex": "(a|b)*"}]


class Case:
    """B rows over V entries, every sampler path among the rows, guided rows (each in a state
    reached by a random allowed walk, or accepting, or with a single allowed token) mixed with
    unguided ones - without a slot, or with a slot that follows no guide."""

    def __init__(self, B, V, dtype, stride, seed, pen):
        ops.native()
        r = random.Random(seed)
        g = torch.Generator().manual_seed(seed)
        self.B, self.V, self.vb = B, V, make_vocab(V)
        x = torch.randint(-128, 129, (B, V), generator=g).float() / 16
        buf = torch.zeros(B, stride, dtype=dtype)
        buf[:, :V] = x.to(dtype)
        assert torch.equal(buf[:, :V].float(), x)
        self.x = x
        self.logits = buf.to(DEV)[:, :V]
        rows = [KINDS[(b + seed) % len(KINDS)] for b in range(B)]
        self.temps = torch.tensor([k[0] for k in rows], device=DEV)
        self.top_k = torch.tensor([k[1] for k in rows], device=DEV, dtype=torch.int32)
        self.top_p = torch.tensor([k[2] for k in rows], device=DEV)
        self.rng = torch.tensor([99 + seed, 5], device=DEV, dtype=torch.int64)
        guides = [compile_guide(s, LIMIT) for s in SPECS] + [compile_guide({"choice": ["Q"]}, LIMIT)]
        n_slots = B + 2
        self.gs = ops.GuideState(n_slots, V, self.vb, EOS, DEV, rows=sum(q.n for q in guides) + 3)
        order = list(range(n_slots))
        r.shuffle(order)
        self.gslots, self.local, self.guide_of = [], {}, {}
        self.allowed = torch.ones(B, V, dtype=torch.bool)
        for b in range(B):
            if b % 4 == 3:
                self.gslots.append(-1)  # no slot
                continue
            slot = order[b]
            self.gslots.append(slot)
            if b % 8 == 5:
                continue  # a slot that follows no guide: state -1
            q = guides[-1] if b == 0 else guides[b % len(SPECS)]  # row 0: the single allowed token "Q"
            exp = expect_mask(q, V)
            toks, s = [], 0
            for _ in range(0 if b == 0 else r.randint(0, 6)):
                ok = [t for t in torch.nonzero(exp[s]).flatten().tolist() if t not in EOS]
                if not ok:
                    break
                t = r.choice(ok)
                toks.append(t)
                s = ref.guide_advance(q.trans, s, self.vb[t])
            self.gs.reset(slot, q, toks)
            assert self.gs.walk(q, toks) == s
            self.local[b], self.guide_of[b] = s, q
            self.allowed[b] = exp[s]
        assert int(self.allowed[0].sum()) == 1
        self.d_gslots = torch.tensor(self.gslots, device=DEV, dtype=torch.int32)
        self.pre = x.masked_fill(~self.allowed, float("-inf")).to(dtype).to(DEV)  # contiguous, -inf prefilled
        self.pen = self.pen_ref = self.d_pslots = None
        if pen:
            self.pen, self.pen_ref = ops.PenaltyState(B + 1, V, DEV), ops.PenaltyState(B + 1, V, DEV)
            pslots = [(-1 if b % 3 == 1 else (b * 7) % (B + 1)) for b in range(B)]
            pslots = [p if pslots.index(p) == i or p < 0 else -1 for i, p in enumerate(pslots)]
            self.d_pslots = torch.tensor(pslots, device=DEV, dtype=torch.int32)
            for b, p in enumerate(pslots):
                if p < 0:
                    continue
                top = torch.topk(x[b].masked_fill(~self.allowed[b], -99.0), 20).indices.tolist()
                args = (top[:8], top[4:16] * 2, [1.0, 2.0, 4.0][b % 3], (b % 5) / 8, (b % 3) / 8)
                self.pen.reset(p, *args)
                self.pen_ref.reset(p, *args)

    def run(self):
        kw = dict(penalties=self.pen, slots=self.d_pslots) if self.pen is not None else {}
        kw_ref = dict(penalties=self.pen_ref, slots=self.d_pslots) if self.pen is not None else {}
        before = self.gs.state.cpu().tolist()
        got = ops.sample(self.logits, self.temps, self.top_k, self.top_p, self.rng.clone(), guide=self.gs,
                         gslots=self.d_gslots, **kw)
        want = ops.sample(self.pre, self.temps, self.top_k, self.top_p, self.rng.clone(), **kw_ref)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        toks = got.cpu().tolist()
        after = self.gs.state.cpu().tolist()
        changed = 0
        for b, slot in enumerate(self.gslots):
            if b not in self.local:
                if slot >= 0:
                    assert after[slot] == -1
                continue
            t, q = toks[b], self.guide_of[b]
            assert bool(self.allowed[b, t])
            rows = self.gs.resident_rows(q)
            if t in EOS:
                assert after[slot] == before[slot]
                continue
            s = ref.guide_advance(q.trans, self.local[b], self.vb[t])
            assert s >= 0 and after[slot] == int(rows[s])
            changed += after[slot] != before[slot]
        used = {s for s in self.gslots if s >= 0}
        assert all(after[s] == before[s] for s in range(self.gs.slots) if s not in used)
        if self.pen is not None:
            assert torch.equal(self.pen.table, self.pen_ref.table)
        return changed


@pytest.mark.parametrize("pen", [False, True])
@pytest.mark.parametrize("B,V,dtype,stride", [
    (1, 1000, torch.bfloat16, 1008), (3, 1000, torch.bfloat16, 1003), (3, 1000, torch.float32, 1000),
    (64, 1000, torch.bfloat16, 1000), (64, 1000, torch.float32, 1001), (130, 1000, torch.bfloat16, 1008),
    (130, 1000, torch.bfloat16, 1005), (3, 32776, torch.bfloat16, 32776), (3, 32776, torch.float32, 32776),
    (5, 32776, torch.bfloat16, 32779)])
def test_guided_sampler_equals_prefilled_logits(B, V, dtype, stride, pen):
    # V = 32776 with B <= 5 is split into 4 parts of 8200 entries; a stride that is no multiple of
    # 8 takes the scalar loop, the others the 16-byte loads with one mask byte per load
    changed = 0
    for seed in range(2):  # every sampler path meets every kind of row
        changed += Case(B, V, dtype, stride, seed, pen).run()
    assert changed > 0


def test_captured_graph_advances_the_state_every_replay():
    ops.native()
    V, B = 1000, 3
    vb = make_vocab(V)
    q = compile_guide({"regex": "[abc]{200}x"}, LIMIT)
    gs = ops.GuideState(B, V, vb, EOS, DEV, rows=q.n)
    rows = gs.load(q)
    g = torch.Generator().manual_seed(0)
    logits = (torch.randint(-128, 129, (B, V), generator=g).float() / 16).to(torch.bfloat16).to(DEV)
    temps = torch.tensor([1.0, 0.8, 1.2], device=DEV)
    rng = torch.tensor([7, 0], device=DEV, dtype=torch.int64)
    gslots = torch.tensor([2, -1, 0], device=DEV, dtype=torch.int32)
    out = torch.zeros(B, dtype=torch.int32, device=DEV)

    def body():
        ops.sample(logits, temps, None, None, rng, out=out, advance=True, guide=gs, gslots=gslots)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    gs.reset(2, q, [])
    gs.reset(0, q, [])
    rng.copy_(torch.tensor([7, 0]))
    local = {2: 0, 0: 0}
    for _ in range(20):
        graph.replay()
        torch.cuda.synchronize()
        toks = out.cpu().tolist()
        for row, slot in ((0, 2), (2, 0)):
            nxt = ref.guide_advance(q.trans, local[slot], vb[toks[row]])
            assert nxt >= 0 and nxt != local[slot]  # an allowed token, and [abc]{200} never stands still
            local[slot] = nxt
        st = gs.state.cpu().tolist()
        assert st[2] == int(rows[local[2]]) and st[0] == int(rows[local[0]]) and st[1] == -1
    assert int(rng[1]) == 20 and min(local.values()) >= 20


def test_eos_draw_leaves_the_state_and_reset_equals_the_walk():
    ops.native()
    V = 1000
    vb = make_vocab(V)
    q = compile_guide({"regex": "(ab)*"}, LIMIT)  # the start state accepts
    gs = ops.GuideState(2, V, vb, EOS, DEV, rows=q.n + 2)
    rows = gs.load(q)
    gs.reset(1, q, [])
    logits = torch.zeros(1, V, device=DEV)
    logits[0, EOS[1]] = 4.0  # greedy: the eos id wins (it is allowed: the state accepts)
    tok = ops.sample(logits, guide=gs, gslots=torch.tensor([1], device=DEV, dtype=torch.int32))
    assert int(tok[0]) == EOS[1] and int(gs.state[1]) == int(rows[0])
    logits[0, EOS[1]] = 0.0
    logits[0, ord("a")] = 3.0
    logits[0, ord("b")] = 5.0  # not allowed in the start state
    tok = ops.sample(logits, guide=gs, gslots=torch.tensor([1], device=DEV, dtype=torch.int32))
    assert int(tok[0]) == ord("a") and int(gs.state[1]) == int(rows[ref.guide_advance(q.trans, 0, b"a")])
    # reset: eos ids, ids outside the vocabulary, tokens without bytes and dying tokens are skipped
    ab = next(t for t in range(256, V) if vb[t] == b"ab") if b"ab" in vb[256:] else None
    toks = [ord("a"), ord("b"), EOS[0], 257, V + 7, -1, ord("x"), ord("a")] + ([ab] if ab is not None else [])
    s = 0
    for t in toks:
        if 0 <= t < V and t not in EOS and vb[t]:
            n = ref.guide_advance(q.trans, s, vb[t])
            s = n if n >= 0 else s
    gs.reset(0, q, toks)
    assert gs.walk(q, toks) == s and int(gs.state[0]) == int(rows[s]) and int(gs.state[1]) != -1
    gs.release(1)
    assert int(gs.state[1]) == -1 and gs.slots_in_use == 1
