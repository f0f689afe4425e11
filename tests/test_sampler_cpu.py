"""The sampler's reference kept set (ops/reference.py ``sample_keep``) on rows with known answers,
the CPU sampling path that is built on it, and the numpy model of the kernel's noise that
tests/test_sampler_gpu.py replays the HIP sampler with."""
import math

import numpy as np
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref
from test_sampler_gpu import gumbel, row_key

NINF = float("-inf")


def kept(row, T, k, p):
    return torch.nonzero(ref.sample_keep(torch.tensor(row), T, k, p)).flatten().tolist()


def test_keep_top_k_with_ties():
    row = [1.0, 5.0, 3.0, 3.0, 0.0, 3.0]
    assert kept(row, 1.0, 1, 1.0) == [1]
    assert kept(row, 1.0, 2, 1.0) == [1, 2, 3, 5], "ties at the k-th value are kept"
    assert kept(row, 0.5, 4, 1.0) == [1, 2, 3, 5]
    assert kept(row, 1.0, 5, 1.0) == [0, 1, 2, 3, 5]
    for k in (0, 6, 7):  # no top-k
        assert kept(row, 1.0, k, 1.0) == [0, 1, 2, 3, 4, 5]


def test_keep_top_p_either_side_of_a_cumulative_mass():
    row = [math.log(0.1), math.log(0.4), math.log(0.2), math.log(0.3)]  # masses 0.4, 0.7, 0.9, 1
    assert kept(row, 1.0, 0, 0.39) == [1]
    assert kept(row, 1.0, 0, 0.41) == [1, 3]
    assert kept(row, 1.0, 0, 0.69) == [1, 3]
    assert kept(row, 1.0, 0, 0.71) == [1, 2, 3]
    assert kept(row, 1.0, 0, 0.91) == [0, 1, 2, 3]
    assert kept(row, 1.0, 0, 1.0) == [0, 1, 2, 3]
    assert kept(row, 1.0, 0, 0.0) == [1], "the largest value is always kept"
    # T = 0.5 squares the masses: 1, 16, 4, 9 of 30 -> cumulative 0.533, 0.833, 0.967
    assert kept(row, 0.5, 0, 0.5) == [1]
    assert kept(row, 0.5, 0, 0.6) == [1, 3]
    assert kept(row, 0.5, 0, 0.9) == [1, 2, 3]


def test_keep_top_p_ties_at_the_last_kept_value():
    row = [math.log(0.25)] * 2 + [math.log(0.5)]  # masses 0.5, 0.75, 1
    assert kept(row, 1.0, 0, 0.6) == [0, 1, 2], "both tokens of the boundary value are kept"
    assert kept(row, 1.0, 0, 0.4) == [2]


def test_keep_top_p_is_over_the_top_k_survivors():
    row = [math.log(0.1), math.log(0.4), math.log(0.2), math.log(0.3)]
    # top-2 survivors renormalise to 4/7 and 3/7: p = 0.5 keeps one of them, p = 0.6 both,
    # though over the whole row p = 0.6 would keep two and p = 0.5 as well
    assert kept(row, 1.0, 2, 0.5) == [1]
    assert kept(row, 1.0, 2, 0.6) == [1, 3]
    assert kept(row, 1.0, 3, 0.8) == [1, 2, 3]  # 4/9, 7/9, 1
    assert kept(row, 1.0, 3, 0.75) == [1, 3]


def test_keep_never_keeps_minus_inf():
    row = [NINF, 2.0, NINF, 1.0, 0.0, NINF]
    assert kept(row, 1.0, 0, 1.0) == [1, 3, 4]
    assert kept(row, 1.0, 2, 1.0) == [1, 3]
    assert kept(row, 1.0, 4, 1.0) == [1, 3, 4], "fewer finite values than k"
    assert kept(row, 1.0, 5, 0.95) == [1, 3, 4]
    assert kept(row, 1.0, 0, 0.7) == [1, 3]  # masses 0.665, 0.910, 1
    assert kept(row, 1.0, 0, 0.6) == [1]


def test_cpu_sampler_draws_inside_the_kept_set():
    B, V = 24, 503
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(B, V, generator=g) * 3
    logits[torch.rand(B, V, generator=g) < 0.2] = NINF
    kinds = [(0.7, 5, 1.0), (1.0, 0, 0.8), (1.3, 50, 0.8), (1.0, 0, 1.0), (0.0, 3, 0.5), (2.0, 1, 1.0)]
    temps = torch.tensor([kinds[r % 6][0] for r in range(B)])
    ks = torch.tensor([kinds[r % 6][1] for r in range(B)], dtype=torch.int32)
    ps = torch.tensor([kinds[r % 6][2] for r in range(B)])
    keep = [ref.sample_keep(logits[r], float(temps[r]), int(ks[r]), float(ps[r])) if temps[r] > 0 else None
            for r in range(B)]
    seen = [set() for _ in range(B)]
    for step in range(40):
        tok = ops.sample(logits, temps, ks, ps, torch.tensor([3, step]))
        for r in range(B):
            seen[r].add(int(tok[r]))
    for r in range(B):
        if keep[r] is None:
            assert seen[r] == {int(logits[r].argmax())}
        else:
            assert all(bool(keep[r][t]) for t in seen[r]), f"row {r} drew outside its kept set"
    assert all(len(seen[r]) > 1 for r in range(B) if kinds[r % 6][:2] == (1.0, 0)), "the draws vary"
    assert all(seen[r] == {int(logits[r].argmax())} for r in range(B) if int(ks[r]) == 1)


def test_noise_model_range_and_mean():
    """The kernel states its noise lies in [-log(16.64), 16.64] = [-2.81, 16.64]; standard Gumbel
    noise has the Euler-Mascheroni constant as its mean."""
    n = 1 << 20
    noise = gumbel(row_key(0, 0, 0), n)
    assert noise.shape == (n,) and np.isfinite(noise).all()
    assert noise.min() >= -math.log(16.64) and noise.max() <= 16.64
    assert abs(noise.mean() - 0.5772156649) < 0.01
    other = gumbel(row_key(0, 0, 1), n)
    assert abs(other.mean() - 0.5772156649) < 0.01 and not np.array_equal(noise, other)
    # the extremes of the 23-bit hash, by the formula
    w = (np.array([0.0, 8388607.0]) + 0.5) / 8388608.0
    assert np.allclose(-np.log(-np.log1p(-w)), [24 * math.log(2), -math.log(24 * math.log(2))], atol=1e-6)
