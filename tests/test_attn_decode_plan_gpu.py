"""Every compiled form of paged decode attention, launched once per instantiation: each row of
ops.PD_FORMS (kPdForms, ops/csrc/paged_decode_forms.h) at TW = 32 and at TW = 64, unsplit and at
S = 3, a fused row with the in-launch merge and with the reduce launch.

One batch, Hkv = 2 and Hq = 2 G, lengths [0, 1, 17, 128, 129, 257, 300] over a shuffled block
table: a padding row, a single token, a block edge and the chunk edges of both TW (4 x 32 = 128 and
4 x 64 = 256 tokens per chunk).  At S = 3 the 300-token row has three valid splits at TW = 32 and
two at TW = 64 (one split is empty: nvalid < S), the 257-token row three and two, the 129-token row
two and one, and the shorter rows finish in the launch that splits the others.

The D = 128 caches are built as tests/test_kv_fp8_gpu.py builds them - an e4m3 cache from the CPU
reference quantiser and the bf16 cache of its dequantised values - so an fp8 row must equal its
bf16 row bit for bit where both read the same tokens: the unfused rows.  A fused fp8 row folds the
new token as quantised, which its bf16 row does not, so there the exact check is on the cache it
writes (quantize_kv of the row the bf16 kernel writes), as in that file's fused test."""
import math

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
BS, HKV = 16, 2
LENS = [0, 1, 17, 128, 129, 257, 300]
B = len(LENS)
MAX_BLOCKS = (max(LENS) + BS - 1) // BS + 1
NB = B * MAX_BLOCKS + 4
NSLABS = 2
FIELDS = ("err", "form", "tw", "merge", "reduce", "gx", "gy", "gz")


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()


def _close(a, b, what, atol=2e-2, rtol=2e-2):
    a, b = a.float(), b.float()
    bad = (a - b).abs() > atol + rtol * b.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} off, max abs diff {float((a - b).abs().max()):.4g}"


@pytest.fixture(scope="module")
def world():
    """Block table, lengths and, per head dim, the caches - left unchanged by the tests (the fused
    cases write into clones) - plus the references computed so far, one per row of the table."""
    g = torch.Generator(device="cpu").manual_seed(19)
    bt = torch.randperm(NB, generator=g)[: B * MAX_BLOCKS].view(B, MAX_BLOCKS).to(torch.int32)
    lens = torch.tensor(LENS, dtype=torch.int32)
    last = (lens - 1).clamp(min=0).long()
    slots = (bt[torch.arange(B), last // BS].long() * BS + last % BS).to(torch.int32)
    slots[lens == 0] = -1  # the padding row writes nothing
    w = {"bt": bt.to(DEV), "lens": lens.to(DEV), "pos": last.to(torch.int32).to(DEV), "slots": slots.to(DEV), "ref": {}}
    all_slots = torch.arange(NB * BS, dtype=torch.int32)
    k = torch.randn(NB * BS, HKV, 128, generator=g).to(torch.bfloat16)
    v = torch.randn(NB * BS, HKV, 128, generator=g).to(torch.bfloat16)
    v[::7] *= 0.02  # token scales that differ inside one block
    k[::5] *= 0.05
    k8, v8, sc = (t[0] for t in ops.kv_cache_alloc(1, NB, HKV, 128, F8, "cpu"))
    ref.write_kv_cache(k, v, k8, v8, all_slots, sc)  # the CPU reference quantiser
    kd, vd = (t[0] for t in ops.kv_cache_alloc(1, NB, HKV, 128, torch.bfloat16, "cpu"))
    ref.write_kv_cache(ops.dequantize_kv(*ops.quantize_kv(k)), ops.dequantize_kv(*ops.quantize_kv(v)), kd, vd, all_slots)
    w[(128, 1)] = (k8.to(DEV), v8.to(DEV), sc.to(DEV))
    w[(128, 0)] = (kd.to(DEV), vd.to(DEV), None)
    k64, v64 = (t[0] for t in ops.kv_cache_alloc(1, NB, HKV, 64, torch.bfloat16, "cpu"))
    ref.write_kv_cache(torch.randn(NB * BS, HKV, 64, generator=g).to(torch.bfloat16),
                       torch.randn(NB * BS, HKV, 64, generator=g).to(torch.bfloat16), k64, v64, all_slots)
    w[(64, 0)] = (k64.to(DEV), v64.to(DEV), None)
    for D in (64, 128):
        w["cs", D] = ref.rope_cos_sin(4096, D, 500000.0, None, device=DEV)
    return w


def _plan_is(row, tw, D, hq, S, fused, f8, merge):
    p = dict(zip(FIELDS, ops.native().paged_decode_plan(D, hq, HKV, B, S, fused, f8, merge, tw)))
    assert (p["err"], p["form"], p["tw"]) == (0, row, tw), p
    assert (p["gx"], p["gy"], p["gz"]) == (S, HKV, B)
    assert (p["merge"], p["reduce"]) == (int(merge and S > 1), int(S > 1 and not merge))


def _unfused(world, row, tw, D, G, f8):
    hq, scale = HKV * G, 1.0 / math.sqrt(D)
    kc, vc, sc = world[(D, f8)]
    g = torch.Generator(device="cpu").manual_seed(100 + row)
    q = torch.randn(B, hq * D, generator=g).to(torch.bfloat16).to(DEV)
    if row not in world["ref"]:
        world["ref"][row] = ref.paged_decode(q.cpu(), kc.cpu(), vc.cpu(), world["bt"].cpu(), world["lens"].cpu(), hq,
                                             HKV, D, scale, kv_scale=None if sc is None else sc.cpu())
    for S in (1, 3):
        _plan_is(row, tw, D, hq, S, False, bool(f8), False)
        y = ops.paged_decode(q, kc, vc, world["bt"], world["lens"], hq, HKV, D, scale, splits=S, kv_scale=sc)
        torch.cuda.synchronize()
        _close(y.cpu(), world["ref"][row], f"row {row} TW {tw} S {S} vs the fp32 reference")
        assert torch.all(y[0] == 0), "the zero-length row is zeros"
        if f8:  # bit for bit the bf16 row over the dequantised cache
            kd, vd, _ = world[(D, 0)]
            _plan_is(ops.PD_FORMS.index((D, G, 0, 0)), tw, D, hq, S, False, False, False)
            r = ops.paged_decode(q, kd, vd, world["bt"], world["lens"], hq, HKV, D, scale, splits=S)
            torch.cuda.synchronize()
            assert torch.equal(y, r), f"row {row} TW {tw} S {S}: {int((y != r).sum())} of {y.numel()} outputs differ"


def _fused(world, row, tw, D, G, f8, monkeypatch):
    hq, scale = HKV * G, 1.0 / math.sqrt(D)
    n = (hq + 2 * HKV) * D
    cs, bt, lens, pos, slots = world["cs", D], world["bt"], world["lens"], world["pos"], world["slots"]
    g = torch.Generator(device="cpu").manual_seed(200 + row)
    slabs = (torch.randn(NSLABS, B, n, generator=g) * 0.5).to(DEV).reshape(-1)

    def cache():
        kc, vc, sc = world[(D, f8)]
        return kc.clone(), vc.clone(), None if sc is None else sc.clone()

    def run(S, ws):
        c = cache()
        y = ops.paged_decode_fused(slabs, NSLABS, pos, cs, slots, c[0], c[1], bt, lens, hq, HKV, D, scale,
                                   workspace=ws, splits=S, kv_scale=c[2])
        torch.cuda.synchronize()
        return y, c

    # rope_and_cache from the slabs, then the unfused kernel: the output and the cache to match
    c2 = cache()
    qkv = torch.empty(B, n, device=DEV, dtype=torch.bfloat16)
    ops.rope_and_cache(qkv, pos, cs, c2[0], c2[1], slots, hq, HKV, D, partial=slabs, nslabs=NSLABS, kv_scale=c2[2])
    if row not in world["ref"]:
        world["ref"][row] = ref.paged_decode(qkv.cpu(), c2[0].cpu(), c2[1].cpu(), bt.cpu(), lens.cpu(), hq, HKV, D,
                                             scale, kv_scale=None if c2[2] is None else c2[2].cpu())
    ws = ops.decode_workspace(B, hq, D, device=DEV, Hkv=HKV)
    for S in (1, 3):
        _plan_is(row, tw, D, hq, S, True, bool(f8), True)
        y, c = run(S, ws)
        what = f"row {row} TW {tw} S {S}"
        assert int(ws[2].abs().sum()) == 0, f"{what}: counters not reset"
        r = ops.paged_decode(qkv, c2[0], c2[1], bt, lens, hq, HKV, D, scale, splits=S, kv_scale=c2[2])
        torch.cuda.synchronize()
        if f8:  # codes and scales: what rope_and_cache's quantiser writes for the same token
            for a, b_, nm in zip(c, c2, ("k codes", "v codes", "scales")):
                assert torch.equal(a.float(), b_.float()), f"{what}: {nm} differ"
        else:
            _close(c[0], c2[0], f"{what}: k cache", atol=1e-2, rtol=1e-2)
            _close(c[1], c2[1], f"{what}: v cache", atol=1e-2, rtol=1e-2)
        _close(y, r, f"{what}: fused vs rope_and_cache + paged_decode")
        _close(y.cpu(), world["ref"][row], f"{what}: fused vs the fp32 reference")
        assert torch.all(y[0] == 0), "the zero-length row is zeros"
        if S == 1:
            continue
        # merge on, a second time back to back (the counters must have been left at zero), and off
        y2, c_2 = run(S, ws)
        assert int(ws[2].abs().sum()) == 0, f"{what}: counters not reset by the second launch"
        monkeypatch.setattr(ops, "DECODE_MERGE", False)
        _plan_is(row, tw, D, hq, S, True, bool(f8), False)
        y3, c_3 = run(S, ws)
        monkeypatch.setattr(ops, "DECODE_MERGE", True)
        for other, oc, nm in ((y2, c_2, "the second merge launch"), (y3, c_3, "the reduce launch")):
            assert torch.equal(y, other), f"{what}: output differs from {nm}"
            assert torch.equal(c[0].view(torch.uint8), oc[0].view(torch.uint8)), f"{what}: k cache differs from {nm}"
            assert torch.equal(c[1].view(torch.uint8), oc[1].view(torch.uint8)), f"{what}: v cache differs from {nm}"
    if f8:  # exactly quantize_kv of the row the bf16 fused kernel writes for the same slabs
        kd, vd, _ = world[(D, 0)]
        cb = (kd.clone(), vd.clone())
        ops.paged_decode_fused(slabs, NSLABS, pos, cs, slots, cb[0], cb[1], bt, lens, hq, HKV, D, scale, workspace=ws,
                               splits=1)
        torch.cuda.synchronize()
        live = slots[slots >= 0].long()
        blk, off = live // BS, live % BS
        k_row = cb[0][blk, :, :, off, :].reshape(live.numel(), HKV, D).cpu()
        v_row = cb[1][blk, :, :, ref.v_perm(off)].cpu()
        want = tuple(t.cpu().clone() for t in world[(D, 1)])
        ref.write_kv_cache(k_row, v_row, want[0], want[1], live.to(torch.int32).cpu(), want[2])
        for a, b_, nm in zip(c, want, ("k codes", "v codes", "scales")):
            assert torch.equal(a.cpu().float(), b_.float()), f"row {row} TW {tw}: {nm} are not quantize_kv of the bf16 row"


@pytest.mark.parametrize("tw", [32, 64])
@pytest.mark.parametrize("row", range(len(ops.PD_FORMS)), ids=lambda i: "D{}-G{}-fused{}-f8{}".format(*ops.PD_FORMS[i]))
def test_every_row_at_both_chunk_widths(world, row, tw, monkeypatch):
    D, G, fused, f8 = ops.PD_FORMS[row]
    ops.native().decode_tw_force(tw)
    try:
        if fused:
            _fused(world, row, tw, D, G, f8, monkeypatch)
        else:
            _unfused(world, row, tw, D, G, f8)
    finally:
        ops.native().decode_tw_force(0)


def test_the_launcher_refuses_what_has_no_row(world):
    D, scale = 128, 1.0 / math.sqrt(128)
    kc, vc, _ = world[(D, 0)]
    q = torch.zeros(B, 6 * D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):  # G = 3
        ops.paged_decode(q, kc, vc, world["bt"], world["lens"], 6, HKV, D, scale, splits=1)
    hq = 16 * HKV
    slabs = torch.zeros(NSLABS * B * (hq + 2 * HKV) * D, device=DEV)
    with pytest.raises(RuntimeError):  # fused G = 16; the unfused kernel has the form
        ops.paged_decode_fused(slabs, NSLABS, world["pos"], world["cs", D], world["slots"], kc.clone(), vc.clone(),
                               world["bt"], world["lens"], hq, HKV, D, scale, splits=1)
    torch.cuda.synchronize()
