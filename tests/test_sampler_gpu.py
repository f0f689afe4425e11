"""ops.sample against an exact model of the op: the kept set of ops/reference.py ``sample_keep``
(float64: top-k, then top-p over the survivors, ties kept) and a numpy replay of the kernel's
documented noise, a function of (seed, counter, row, index).

The expected token of a sampled row is ``argmax over the kept set of (x / T + gumbel)``, lowest
index on ties; of a greedy row, the lowest index of the maximum.  The kernel takes the fast log and
scales in fp32, so its score is within about 1e-5 of the model's (1 ULP of the hardware log on
noise of magnitude <= 17, fp32 rounding of |x / T| <~ 100): a row whose two best model scores are
closer than ``SKIP`` is not compared, and every case asserts that this leaves out at most 1 row in
32.  The inputs are given a clear kept-set boundary first (asserted before the kernel runs):
the k-th and (k+1)-th scaled values differ by more than ``GAP``, and each p lies halfway between
two consecutive cumulative masses of the reference, at a boundary token of probability >= 1e-3."""
import functools

import numpy as np
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SKIP = 1e-3  # two best scores closer than this: the row is not compared (at most 1 row in 32)
GAP = 1e-4   # least distance of the k-th and the (k+1)-th scaled value of a filtered row
M64 = (1 << 64) - 1


# ------------------------------------------------------------- the kernel's noise, in numpy

def mix64(z: int) -> int:
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def row_key(seed: int, counter: int, row: int) -> int:
    return mix64((seed & M64) ^ mix64(((counter & M64) * 0x100000001b3 + row * 0x9e3779b97) & M64))


def fmix32(h: np.ndarray) -> np.ndarray:
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85ebca6b)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xc2b2ae35)
    return h ^ (h >> np.uint32(16))


def gumbel(key: int, n: int) -> np.ndarray:
    """Noise of indices [0, n) under ``key``: -log(-log(1 - w)), w = (23-bit hash + 0.5) / 2^23."""
    i = np.arange(n, dtype=np.uint32)
    h = fmix32(fmix32(i * np.uint32(0x9e3779b9) ^ np.uint32(key & 0xffffffff)) + np.uint32(key >> 32))
    w = ((h >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0
    return -np.log(-np.log1p(-w))


# ------------------------------------------------------------- the model of one call

def keep_sets(x: torch.Tensor, temps, ks, ps) -> list:
    """ref.sample_keep of every sampled row of x [B, V] (CPU); None for a greedy row."""
    return [ref.sample_keep(x[r], temps[r], ks[r], ps[r]).numpy() if temps[r] > 0 else None
            for r in range(x.shape[0])]


def model(x: torch.Tensor, temps, keeps, seed: int, counter: int):
    """Expected token of every row and the distance of its two best scores (inf: nothing to tie)."""
    xd = x.double().numpy()
    B, V = xd.shape
    tok, margin = np.empty(B, np.int64), np.full(B, np.inf)
    for r in range(B):
        if keeps[r] is None:
            tok[r] = int(np.argmax(xd[r]))  # first index of the maximum
            continue
        score = np.where(keeps[r], xd[r] * (1.0 / temps[r]) + gumbel(row_key(seed, counter, r), V), -np.inf)
        tok[r] = int(np.argmax(score))
        if V > 1:
            second, best = np.partition(score, V - 2)[V - 2:]
            margin[r] = best - second
    return tok, margin


def assert_topk_boundary(x: torch.Tensor, temps, ks):
    """Input check: the k-th and (k+1)-th scaled values of every top-k row differ by more than GAP."""
    V = x.shape[1]
    for r in range(x.shape[0]):
        if temps[r] > 0 and 0 < ks[r] < V:
            top = torch.topk(x[r].double() * (1.0 / temps[r]), ks[r] + 1).values
            assert float(top[-2] - top[-1]) > GAP, f"row {r}: no clear top-{ks[r]} boundary"


def pick_p(row: torch.Tensor, T: float, k: int, target: float) -> float:
    """A p near ``target`` halfway between two consecutive cumulative masses of the reference
    distribution (softmax of the top-k survivors of row / T, sorted descending), whose boundary
    token has probability >= 1e-3 and is the last of its value (or GAP above the next value)."""
    v = row.double() * (1.0 / T)
    w = torch.softmax(v.masked_fill(~ref.sample_keep(row, T, k, 1.0), float("-inf")), -1)
    sw, order = torch.sort(w, descending=True)
    sv, cum = v[order], torch.cumsum(sw, 0)
    n = max(2, min(int((cum < target).sum()) + 1, row.numel() - 1))  # smallest prefix that reaches target
    gap = sv[:-1] - sv[1:]  # gap[n - 1]: from the last token of a prefix of n to the next one
    ok = (sw[:-1] >= 1e-3) & ((gap == 0) | (gap > GAP))
    ok[0] = False  # a prefix of at least 2
    n = int(torch.nonzero(ok[:n]).max()) + 1  # raises if the row has no such boundary
    assert n >= 2 and float(sw[n - 1]) >= 1e-3 and not 0.0 < float(sv[n - 1] - sv[n]) <= GAP, "no clear top-p boundary"
    return float(np.float32((cum[n - 2] + cum[n - 1]) / 2))


def f32(v) -> float:
    return float(np.float32(v))


def run(xg: torch.Tensor, temps, ks, ps, rng=None) -> np.ndarray:
    t = torch.tensor(temps, dtype=torch.float32, device=DEV)
    k = torch.tensor(ks, dtype=torch.int32, device=DEV)
    p = torch.tensor(ps, dtype=torch.float32, device=DEV)
    r = None if rng is None else torch.tensor(rng, dtype=torch.int64, device=DEV)
    tok = ops.sample(xg, t, k, p, r).cpu().numpy().astype(np.int64)
    assert tok.min() >= 0 and tok.max() < xg.shape[1], f"token outside [0, V): {tok.min()} .. {tok.max()}"
    return tok


def compare(tok: np.ndarray, exp: np.ndarray, margin: np.ndarray, what: str):
    use = margin > SKIP
    assert 32 * int((~use).sum()) <= len(tok), f"{what}: {int((~use).sum())} of {len(tok)} rows have no clear winner"
    bad = np.nonzero(use & (tok != exp))[0]
    assert bad.size == 0, f"{what}: rows {bad.tolist()} drew {tok[bad].tolist()}, the model {exp[bad].tolist()}"


def distinct_top(x: torch.Tensor, r: int, n: int, step: float = 0.125):
    """Overwrite the n largest entries of row r, in their order, with a ladder of multiples of
    ``step`` (exact and distinct in bf16 below 32) that ends one step above the rest of the row:
    close enough to the rest for the mass below the ladder to matter to top-p."""
    top = torch.topk(x[r].float(), min(n + 1, x.shape[1]))
    rest = float(top.values[n]) if n < x.shape[1] else 0.0
    base = (np.ceil(rest / step) + 1) * step
    assert base + step * n < 32
    x[r, top.indices[:n]] = (base + step * torch.arange(n - 1, -1, -1)).to(x.dtype)


# ------------------------------------------------------------- exact replay, mixed batch

V_PAD, V_GPT2 = 50304, 50257  # CausalLM._logits: a [:, :vocab_size] view of the padded logits
# (T, k, p or the target of a chosen p) of consecutive rows, repeated down the batch
KINDS = [(0.0, 5, 0.5), (0.0, 0, 1.0),                           # greedy; the engine's padding row
         (0.1, 0, 1.0), (1.0, 0, 1.0), (3.0, 0, 1.0),            # unfiltered
         (0.7, 1, 1.0), (0.7, 5, 1.0), (1.0, 50, 1.0),           # top-k only
         (1.0, 0, 0.9), (0.7, 0, 0.5),                           # top-p only
         (1.3, 50, 0.8), (0.7, 5, 0.6), (1.0, 50, 0.5)]          # both


@functools.lru_cache(maxsize=None)
def mixed_batch(dtype):
    """(padded device logits, CPU rows as the kernel reads them, temps, ks, ps, kept sets), once per dtype."""
    B = 64
    g = torch.Generator().manual_seed(20)
    full = (torch.randn(B, V_PAD, generator=g) * 3).to(dtype)
    full[:, V_GPT2:] = 100.0  # a read past V wins the row and shows as a token >= V
    temps = [f32(KINDS[r % len(KINDS)][0]) for r in range(B)]
    ks = [KINDS[r % len(KINDS)][1] for r in range(B)]
    ps = [f32(KINDS[r % len(KINDS)][2]) for r in range(B)]
    x = full[:, :V_GPT2]
    for r in range(B):
        if dtype == torch.bfloat16 and temps[r] > 0 and ks[r] > 0:
            distinct_top(x, r, ks[r] + 1)
        if temps[r] > 0 and ps[r] < 1:
            ps[r] = pick_p(x[r].float(), temps[r], ks[r], ps[r])
    xf = x.float()
    assert_topk_boundary(xf, temps, ks)
    return full.to(DEV), xf, temps, ks, ps, keep_sets(xf, temps, ks, ps)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_exact_replay_mixed_batch(dtype):
    """64 rows with interleaved per-row parameters over the engine's padded-vocabulary view (6 parts,
    vector body + scalar tail, stride != V): every token is the model's."""
    full, xf, temps, ks, ps, keeps = mixed_batch(dtype)
    xg = full[:, :V_GPT2]
    assert not xg.is_contiguous() and xg.stride(0) == V_PAD
    for seed, counter in [(1234, 0), (-5, 1 << 40)]:
        tok = run(xg, temps, ks, ps, [seed, counter])
        compare(tok, *model(xf, temps, keeps, seed, counter), f"rng ({seed}, {counter})")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_exact_replay_without_rng(dtype):
    """rng = None draws with the key of (seed 0, counter 0)."""
    full, xf, temps, ks, ps, keeps = mixed_batch(dtype)
    tok = run(full[:, :V_GPT2], temps, ks, ps, None)
    compare(tok, *model(xf, temps, keeps, 0, 0), "rng None")


# ------------------------------------------------------------- small and odd V (one part)

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1, 7, 8, 9, 1023, 1025])
def test_small_and_odd_vocab(V, dtype):
    """B = 5, dense rows and rows of a wider tensor: unfiltered, k = 3, and the settings that must
    take the unfiltered rule (k >= V, p = 1.0 exactly)."""
    B = 5
    g = torch.Generator().manual_seed(100 + V)
    wide = ((V + 7) // 8) * 8 + 8
    full = (torch.randn(B, wide, generator=g) * 2).to(dtype)
    full[:, V:] = 100.0
    x = full[:, :V]
    if dtype == torch.bfloat16 and V > 3:
        for r in range(B):
            distinct_top(x, r, 4, 0.25)
    xf = x.float()
    settings = [("unfiltered", 0.8, 0, 1.0), ("k = 3", 0.8, 3, 1.0), ("k = V", 1.0, V, 1.0),
                ("k > V", 1.0, V + 5, 1.0), ("p = 1", 1.3, 0, 1.0), ("greedy", 0.0, 3, 0.5)]
    for layout, xg in [("dense", x.contiguous().to(DEV)), ("padded", full.to(DEV)[:, :V])]:
        for i, (name, T, k, p) in enumerate(settings):
            temps, ks, ps = [f32(T)] * B, [k] * B, [f32(p)] * B
            assert_topk_boundary(xf, temps, ks)
            keeps = keep_sets(xf, temps, ks, ps)
            if T > 0 and (k >= V or k == 0):
                assert all(kp.all() for kp in keeps), "the unfiltered rule keeps every token"
            tok = run(xg, temps, ks, ps, [77, i])
            compare(tok, *model(xf, temps, keeps, 77, i), f"{layout}, {name}")


# ------------------------------------------------------------- the kept set, read off the draws

def test_kept_set_and_frequencies():
    """4096 identical rows (V = 1000, fp32, T = 2): the set of tokens drawn is exactly the
    reference kept set and their frequencies the renormalised softmax over it, for top-k, top-p,
    and top-p over the top-k survivors.  No use of the noise model."""
    B, V, T = 4096, 1000, 2.0
    row = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 3
    v = row.double() / T
    top8 = torch.softmax(torch.topk(v, 8).values, 0)
    cum_all, cum8 = torch.cumsum(torch.sort(torch.softmax(v, 0), descending=True).values, 0), torch.cumsum(top8, 0)
    cases = [("k = 8", 8, 1.0, 8),
             ("p keeps 6", 0, f32((cum_all[4] + cum_all[5]) / 2), 6),
             ("k = 8, p keeps 5 of them", 8, f32((cum8[3] + cum8[4]) / 2), 5)]
    top9 = torch.topk(v, 9).values
    assert float((top9[:-1] - top9[1:]).min()) > GAP, "the 9 largest values are not clearly apart"
    logits = row.repeat(B, 1).to(DEV)
    for i, (name, k, p, n) in enumerate(cases):
        keep = ref.sample_keep(row, T, k, p)
        want = torch.softmax(v.masked_fill(~keep, float("-inf")), 0)
        assert int(keep.sum()) == n and float(want[keep].min()) >= 0.01, f"{name}: the inputs do not make this case"
        tok = run(logits, [T] * B, [k] * B, [p] * B, [7, i])
        freq = torch.bincount(torch.from_numpy(tok), minlength=V).double() / B
        assert torch.equal(freq > 0, keep), \
            f"{name}: drew {torch.nonzero(freq > 0).flatten().tolist()}, kept set {torch.nonzero(keep).flatten().tolist()}"
        assert torch.allclose(freq, want, atol=0.03), f"{name}: frequencies off by {float((freq - want).abs().max()):.4f}"


# ------------------------------------------------------------- greedy ties

# indices that hold the row's maximum.  Parts of the 50257-wide row are 8384 wide (6 parts); a
# bf16 part is read 8 per thread, 512 per wave, 8192 per pass; [50256, 50257) is the scalar tail.
TIES = [[9000, 100],                      # two parts
        [8384 * 5 + 1, 8384 * 2, 8390],   # three parts
        [8384 + 600, 8384 + 10],          # two waves of one part
        [16768 + 8 * 40 + 2, 16768 + 8 * 3 + 1],  # two threads of one wave
        [16768 + 5, 16768 + 3],           # two lanes of one vector
        [8192 + 5, 5],                    # two passes of one thread
        [50256, 50000],                   # vector body and scalar tail
        [50256, 50255],                   # the last vector and the scalar tail
        [50256]]                          # the scalar tail alone


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_greedy_ties_lowest_index(dtype):
    """The maximum written at several indices: the token is the lowest of them (torch.argmax)."""
    B = 64
    full = torch.randn(B, V_PAD, generator=torch.Generator().manual_seed(3)).to(dtype)
    full[:, V_GPT2:] = 100.0
    want = []
    for r in range(B):
        full[r, TIES[r % len(TIES)]] = 50.0
        want.append(min(TIES[r % len(TIES)]))
    xg = full.to(DEV)[:, :V_GPT2]
    assert want == torch.argmax(full[:, :V_GPT2].float(), -1).tolist()
    assert ops.sample(xg).tolist() == want
    assert ops.sample(xg, torch.zeros(B, device=DEV)).tolist() == want


# ------------------------------------------------------------- masked logits

@pytest.mark.parametrize("mask", [float("-inf"), -1e9], ids=["-inf", "-1e9"])
def test_masked_logits(mask):
    """30 % of each row masked out (V = 32003, 3 parts): the filters see the unmasked values only."""
    B, V = 64, 32003
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, V, generator=g) * 3
    x[torch.rand(B, V, generator=g) < 0.3] = mask
    kinds = [(0.0, 0, 1.0), (1.0, 1, 1.0), (0.7, 5, 1.0), (1.0, 0, 0.8), (1.3, 50, 0.8), (1.0, 0, 1.0)]
    temps = [f32(kinds[r % len(kinds)][0]) for r in range(B)]
    ks = [kinds[r % len(kinds)][1] for r in range(B)]
    ps = [f32(kinds[r % len(kinds)][2]) for r in range(B)]
    for r in range(B):
        if temps[r] > 0 and ps[r] < 1:
            ps[r] = pick_p(x[r], temps[r], ks[r], ps[r])
    assert_topk_boundary(x, temps, ks)
    assert bool((x > mask).any(-1).all())
    keeps = keep_sets(x, temps, ks, ps)
    tok = run(x.to(DEV), temps, ks, ps, [31, 4])
    compare(tok, *model(x, temps, keeps, 31, 4), f"mask {mask}")
    top1 = [r for r in range(B) if ks[r] == 1]
    assert tok[top1].tolist() == torch.argmax(x[top1], -1).tolist(), "k = 1 is the argmax"


# ------------------------------------------------------------- row alignment

def test_rows_off_16_byte_alignment():
    """A bf16 [:, 1:] view: the stride is a multiple of 8 and every row starts 2 bytes off a
    16-byte boundary, so the rows take the scalar loop."""
    B, W = 8, 32768 + 8
    full = (torch.randn(B, W, generator=torch.Generator().manual_seed(13)) * 3).to(torch.bfloat16)
    for r in range(B // 2, B):  # a clear top-5 boundary in half of the rows, bf16 ties in the others
        distinct_top(full[:, 1:], r, 6)
    xg = full.to(DEV)[:, 1:]
    xf = full[:, 1:].float()
    assert xg.stride(0) % 8 == 0 and xg.data_ptr() % 16 == 2
    for i, (name, T) in enumerate([("greedy", 0.0), ("sampled", 1.0), ("sampled", 0.3)]):
        temps, ks, ps = [f32(T)] * B, [0] * (B // 2) + [5] * (B // 2), [1.0] * B
        assert_topk_boundary(xf, temps, ks)
        tok = run(xg, temps, ks, ps, [2, i])
        compare(tok, *model(xf, temps, keep_sets(xf, temps, ks, ps), 2, i), name)
