"""The persistent tile walks of the pipelined bf16 kernels, pinned by BIT equality (the method of tests/test_gpu_exact.py).

igemm2.hip (forward, data gradient, fused 32 -> 32 backward) and wgrad2.hip plan at most 256 (512) persistent workgroups and
walk their items -- (tile, channel block) pairs / tiles -- in one of three ways: one item per workgroup, CONTIGUOUS runs of
two or more items (a workgroup may start in the middle of a tile, the last one is short), or interleaved (tiles b, b + grid,
...).  The shapes of the other kernel-level tests all land on the first or the last; bench.py's bottleneck layers run the
contiguous one.  Every case here states the walk it exists for and asserts it BEFORE launching, from the public host queries
(a literal grid / slab count) and the test's own tile arithmetic, so that a planner change fails the assertion instead of
silently removing the coverage.  first.hip's grid-stride loops (caps of 4096 / 512 workgroups) get their later trips too, counted in each kernel's own units.

Operands are exactly representable (exact_ref.py), the reference is torch's float64 convolution on the host, and every
output element is compared for equality: a tile that is skipped, written twice, or computed with the previous channel
block's weights differs, however small its numerical weight."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import test_gpu_fused_backward as FB
import test_gpu_wgrad_apply_store as AS
from exact_ref import dev, exact_src_host, fdev, host, ints, pow2_weights, same, to_bf16, upload_src

pytestmark = pytest.mark.gpu
BF, XF_RELU = 0, 1     # OCT_DT_BF16, OCT_XF_AFFINE_RELU


@pytest.fixture(scope="module")
def env():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    from retinal_oct_image_segmentation_via_deep_learning_amd import engine as E
    L.lib()
    return L, E


def seed(cid, k=0):
    return zlib.crc32(cid.encode()) + k


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def pad_of(kh, kw):
    return (kh // 2, kw // 2)


def engine_for(E):
    return E.UNetEngine(1, 2, 4, "bf16")


def packed(L, eng, wd, mode, cout, cin, kh, kw):
    from retinal_oct_image_segmentation_via_deep_learning_amd import ops
    if kh == 7:
        return ops.packed(eng, wd, mode, cout, cin, cache=False, kk=(7, 3))
    if kh == 1:
        mode = L.PACK_1X1_FPROP if mode == L.PACK_CONV_FPROP else L.PACK_1X1_DGRAD
    return eng._pack("w", wd, mode, cout, cin)


def kk_of(kh):
    return dict(kh=7, kw=3) if kh == 7 else {}


# ---- forward and data gradient (igemm2.hip) -----------------------------------------------------------------------------------
# id -> (shape (n, h, w, c0, c1, cout) as the kernel sees it, (kh, kw), tile rows, channel blocks, expected grid, dgrad?, split,
#        what it pins).  Forward cases run with the on-load transform and the BatchNorm sums (FPROP packing); data-gradient cases
#        with neither (DGRAD packing: the LDS-DMA variant), `split` channels into the first of two outputs.
CONTIGUOUS = {
    "A": ((3, 112, 416, 32, 0, 32), (3, 3), 16, 1, 137, False, 0, "NT32, 16-row, resident weights; 273 tiles, 2 per workgroup, the last has 1"),
    "B": ((1, 152, 448, 64, 0, 32), (3, 3), 8, 1, 133, False, 0, "NT32, 8-row, streamed weights"),
    "C": ((3, 112, 416, 32, 32, 32), (3, 3), 16, 1, 137, False, 0, "WLDS (concat)"),
    "D": ((1, 152, 448, 32, 0, 64), (3, 3), 8, 1, 133, False, 0, "NT64, resident weights"),
    "E": ((3, 112, 416, 64, 0, 64), (3, 3), 16, 1, 137, False, 0, "NT64, 16-row"),
    "R": ((1, 150, 440, 64, 0, 64), (3, 3), 8, 1, 133, False, 0, "ragged last row and column inside a multi-item walk"),
    "F3": ((1, 88, 256, 96, 0, 192), (3, 3), 8, 3, 132, False, 0, "NT64, 3 blocks, 2 items per workgroup: starts at block 0, 2, 1"),
    "F2": ((1, 152, 448, 32, 0, 256), (3, 3), 8, 2, 178, False, 0, "NT128, 2 blocks, 3 items per workgroup"),
    "F4": ((1, 88, 384, 32, 0, 512), (3, 3), 8, 4, 176, False, 0, "NT128, 4 blocks, 3 items per workgroup (start blocks 0, 3, 2, 1)"),
    "H4": ((1, 128, 512, 32, 0, 512), (3, 3), 8, 4, 256, False, 0, "256 tiles x 4 blocks, 4 per workgroup: the benchmark bottleneck's walk"),
    "CC": ((1, 88, 384, 64, 64, 256), (3, 3), 8, 2, 132, False, 0, "virtual concat across items"),
    "G1": ((1, 152, 448, 64, 0, 128), (3, 3), 8, 1, 133, True, 0, "DMA NT128"),
    "G2": ((1, 152, 448, 64, 0, 64), (3, 3), 8, 1, 133, True, 0, "DMA NT64 (h % 16 = 8 keeps 8-row tiles)"),
    "G3": ((1, 88, 384, 64, 0, 256), (3, 3), 8, 2, 132, True, 0, "DMA, 2 blocks"),
    "G4a": ((1, 152, 448, 64, 0, 128), (3, 3), 8, 1, 133, True, 64, "DMA NT128, split output (concat data gradient)"),
    "G4b": ((1, 152, 448, 64, 0, 64), (3, 3), 8, 1, 133, True, 32, "DMA NT64, split output inside the channel block"),
    "O1": ((1, 152, 448, 64, 0, 64), (1, 1), 8, 1, 133, False, 0, "1X1 NT64"),
    "O2": ((1, 152, 448, 64, 0, 32), (1, 1), 8, 1, 133, False, 0, "1X1 NT32"),
    "O3": ((1, 88, 384, 64, 0, 256), (1, 1), 8, 2, 132, False, 0, "1X1 NT128 x 2 blocks"),
    "K1": ((1, 152, 448, 64, 0, 64), (7, 3), 8, 1, 133, False, 0, "TAPS = 21, NT64"),
    "K2": ((1, 88, 384, 64, 0, 256), (7, 3), 8, 2, 132, False, 0, "TAPS = 21, NT128 x 2 blocks"),
}
# >= 512 tiles, 528 = 2 * 256 + 16: workgroups 0..15 take three tiles, the others two -- on the variants tests/test_gpu_exact.py's
# INTERLEAVED (TILE, WLDS) leaves out
INTERLEAVED = {
    "I1": ((1, 264, 512, 64, 0, 64), (3, 3), 8, 1, 256, True, 0, "DMA NT64, interleaved"),
    "I2": ((1, 264, 512, 32, 0, 256), (3, 3), 8, 2, 256, True, 0, "DMA NT128, interleaved, 2 blocks"),
    "I3": ((1, 264, 512, 64, 0, 64), (1, 1), 8, 1, 256, False, 0, "1X1 NT64, interleaved"),
    "I4": ((1, 264, 512, 64, 0, 256), (1, 1), 8, 2, 256, False, 0, "1X1 NT128, interleaved, 2 blocks"),
}
FWD_CASES = dict(CONTIGUOUS, **INTERLEAVED)


def fwd_desc(L, cid):
    (n, h, w, c0, c1, cout), (kh, kw), _, _, _, dgrad, split, _ = FWD_CASES[cid]
    xf = 0 if dgrad else XF_RELU
    return L.ConvDesc(BF, n, h, w, c0, c1, cout, kh * kw, xf, xf if c1 else 0, 0, 0, split, 0 if dgrad else 1,
                      kh if kh == 7 else 0, kw if kh == 7 else 0, 0, 0, 0)


def assert_fwd_walk(L, cid):
    """the planner's answer is the literal of the table, and by the test's own tile arithmetic that grid is the walk the
    case exists for"""
    (n, h, w, _, _, _), _, th, nblk, grid, _, _, _ = FWD_CASES[cid]
    assert L.lib().oct_conv_stat_blocks(C.byref(fwd_desc(L, cid))) == grid, f"{cid}: the planner no longer answers {grid}"
    ntiles = -(-w // 32) * -(-h // th) * n
    nitems = ntiles * nblk
    assert grid < nitems, f"{cid}: {nitems} items on {grid} workgroups is no multi-item walk"
    if cid in CONTIGUOUS:
        assert ntiles < 512, f"{cid}: {ntiles} tiles walk interleaved"
        per_wg = -(-nitems // 256)
        assert per_wg >= 2 and grid == -(-nitems // per_wg), f"{cid}: {nitems} items, {per_wg} per workgroup"
    else:
        assert ntiles >= 512 and ntiles % 256 != 0 and grid == 256, f"{cid}: {ntiles} tiles"


def fwd_reference(cid):
    """host operands and the float64 reference of one case"""
    (n, h, w, c0, c1, cout), (kh, kw), _, _, _, dgrad, split, _ = FWD_CASES[cid]
    rng = np.random.default_rng(seed(cid))
    pad = pad_of(kh, kw)
    if dgrad:
        # the kernel's input is dY of a layer with `c0` output channels, its output dX with `cout` channels
        wt = pow2_weights(rng, (c0, cout, kh, kw), density=min(0.6, 96.0 / (c0 * kh * kw)))
        dy = ints(rng, (n, c0, h, w))
        ref = torch.nn.grad.conv2d_input((n, cout, h, w), t64(wt), t64(dy), padding=pad).numpy()
        assert np.abs(ref).max() * 8 < 2 ** 22                       # fp32 holds every partial sum exactly
        return dict(wt=wt, dy=dy, ref=ref)
    x0, bn0, x1, bn1, eff = exact_src_host(rng, n, h, w, c0, c1, True)
    # about 96 non-zero weights per output channel, +-1 or +-0.5: with inputs in halves every term is a multiple of 1/4
    wt = pow2_weights(rng, (cout, c0 + c1, kh, kw), density=min(0.6, 96.0 / ((c0 + c1) * kh * kw)), kmin=-1)
    ref = torch.nn.functional.conv2d(t64(eff), t64(wt), padding=pad).numpy()
    assert np.abs(ref).max() * 8 < 2 ** 22
    # the BatchNorm sum of a channel: every partial sum, in any order, is below 2^24 multiples of 1/4
    assert np.abs(ref).sum(axis=(0, 2, 3)).max() * 4 < 2 ** 24
    return dict(src=(x0, bn0, x1, bn1), wt=wt, ref=ref)


@pytest.mark.parametrize("cid", list(FWD_CASES))
def test_forward_and_dgrad_walks_bit_exact(env, cid):
    L, E = env
    (n, h, w, c0, c1, cout), (kh, kw), _, _, grid, dgrad, split, _ = FWD_CASES[cid]
    assert_fwd_walk(L, cid)
    r = fwd_reference(cid)
    eng = engine_for(E)
    if dgrad:
        wp = packed(L, eng, fdev(r["wt"]), L.PACK_CONV_DGRAD, c0, cout, kh, kw)
        c_a = split if split else cout
        d0 = torch.full((n, h, w, c_a), float("nan"), dtype=torch.bfloat16, device="cuda")
        d1 = torch.full((n, h, w, cout - split), float("nan"), dtype=torch.bfloat16, device="cuda") if split else None
        eng._conv(E.Src(dev(r["dy"]), c0), wp, cout, kh * kw, n, h, w, d0, y1=d1, split=split, **kk_of(kh))
        torch.cuda.synchronize()
        ref = to_bf16(r["ref"])
        same(host(d0), ref[:, :c_a], f"{cid}: dgrad" + (" part 0" if split else ""))
        if split:
            same(host(d1), ref[:, split:], f"{cid}: dgrad part 1 (concat split)")
        return
    src = upload_src(E, c0, c1, *r["src"])
    wp = packed(L, eng, fdev(r["wt"]), L.PACK_CONV_FPROP, cout, c0 + c1, kh, kw)
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    part = torch.full((grid, 2, cout), float("nan"), dtype=torch.float32, device="cuda")
    assert eng._stat_blocks(cout, n, h, w, src, kh * kw, **kk_of(kh)) == grid
    eng._conv(src, wp, cout, kh * kw, n, h, w, y, stats=part, **kk_of(kh))
    torch.cuda.synchronize()
    ref = r["ref"]
    same(host(y), to_bf16(ref), f"{cid}: fprop (bf16 store of the exact sum)")
    assert not bool(torch.isnan(part).any()), f"{cid}: a row of the partial sums was not written"
    s = part.double().sum(0).cpu().numpy()
    same(s[0], ref.sum(axis=(0, 2, 3)), f"{cid}: sum(y) from the fp32 accumulators")
    np.testing.assert_allclose(s[1], (ref ** 2).sum(axis=(0, 2, 3)), rtol=1e-5, atol=1e-2)


# ---- fused 32 -> 32 backward (igemm2.hip, FUSE) ----------------------------------------------------------------------------------
# (n, h, w) -> blocks: 266 / 264 8-row tiles, two per workgroup.  Operands, references, comparisons and tolerances are those of
# tests/test_gpu_fused_backward.py, run at these shapes.
FUSED = {(1, 152, 448): 133, (3, 88, 256): 132}


def assert_fused_walk(L, shape):
    n, h, w = shape
    blocks = FUSED[shape]
    assert L.lib().oct_conv_backward_fused_blocks(C.byref(FB.desc(L, n, h, w))) == blocks
    ntiles = (w // 32) * (h // 8) * n
    assert blocks < ntiles < 512 and blocks == -(-ntiles // 2), f"{ntiles} tiles on {blocks} workgroups is not the contiguous walk"


@pytest.mark.parametrize("shape", list(FUSED))
def test_fused_backward_contiguous_walk_bit_exact(env, shape):
    assert_fused_walk(env[0], shape)
    FB.test_fused_backward_bit_exact(env, shape)


@pytest.mark.parametrize("shape", list(FUSED))
def test_fused_backward_contiguous_walk_random_operands(env, shape):
    assert_fused_walk(env[0], shape)
    FB.test_fused_backward_random_operands(env, shape)


# ---- weight gradients (wgrad2.hip) ------------------------------------------------------------------------------------------
# id -> (shape (n, h, w, cin, cout), (kh, kw), tile rows, channel-block pairs side by side, workgroup-column cap, slabs per
#        column, expected slabs, what it pins).  cap = (512 or 256) / pairs; the walk is contiguous for cap < ntiles < 2 * cap.
WGRAD_CASES = {
    "w3_64x64": ((1, 152, 448, 64, 64), (3, 3), 8, 1, 256, 1, 133, "3x3, 64 x 64 blocks: 266 tiles, 2 per workgroup"),
    "w3_32x64": ((1, 152, 448, 64, 32), (3, 3), 8, 1, 256, 2, 266, "3x3, 32 x 64 pairs"),
    "w3_64x32": ((1, 152, 448, 32, 64), (3, 3), 8, 1, 256, 2, 266, "3x3, 64 x 32 pairs"),
    "w3_32x32": ((3, 112, 416, 32, 32), (3, 3), 16, 1, 256, 4, 548, "3x3, 32 x 32, 16-row: 273 tiles, the last workgroup has 1"),
    "w3_128": ((1, 56, 384, 128, 128), (3, 3), 8, 4, 64, 1, 42, "3x3, 128 -> 128: 84 tiles, column cap 64"),
    "w3_256": ((1, 24, 224, 256, 256), (3, 3), 8, 16, 16, 1, 11, "3x3, 256 -> 256: 21 tiles, cap 16, the last workgroup has 1"),
    "w1_128x128": ((1, 88, 384, 128, 128), (1, 1), 4, 1, 256, 1, 132, "1x1, 128 x 128 blocks, 4-row: 264 tiles"),
    "w1_128x64": ((1, 88, 384, 64, 128), (1, 1), 4, 1, 256, 1, 132, "1x1, 128 x 64 blocks"),
    "w1_64x64": ((1, 152, 448, 64, 64), (1, 1), 8, 1, 256, 1, 133, "1x1, 64 x 64 blocks"),
    "w1_32x32": ((3, 112, 416, 32, 32), (1, 1), 8, 1, 512, 4, 1092, "1x1, 32 x 32: 546 tiles, cap 512"),
    "w73": ((1, 152, 448, 64, 64), (7, 3), 8, 1, 256, 1, 133, "7x3, atomics only: two nine-tap launches and one three-tap launch, all three on 133 columns (W73_STAGES)"),
    "w3_ragged": ((1, 150, 440, 64, 64), (3, 3), 8, 1, 256, 1, 133, "3x3 RAGGED instantiation: ragged last row and column"),
}
ATOMICS_ONLY = {"w73"}
# The slab query answers for the nine-tap launches of the 7x3 weight gradient; the three-tap launch sizes its own grid by its
# own, smaller stage: bytes of a 64 x 64 stage = 2 input tiles of (rows + halo) x 34 x 64 + 2 dY tiles of 8 x 32 x 64.  The
# column cap is 512 only where four stages fit the 160-KB LDS -- neither does, so every launch walks 266 tiles on 133 columns.
W73_STAGES = {9: 2 * (8 + 2) * 34 * 64 + 2 * 8 * 32 * 64, 3: 2 * 8 * 34 * 64 + 2 * 8 * 32 * 64}


def wgrad_desc(L, shape, kh, kw, partials, c0=None, c1=0, xf0=XF_RELU, xf1=0):
    n, h, w, cin, cout = shape
    return L.WgradDesc(BF, n, h, w, cin if c0 is None else c0, c1, cout, kh * kw, xf0, xf1, 0, kh if kh == 7 else 0, kw if kh == 7 else 0,
                       0, 0, 0, 0, partials)


def assert_wgrad_walk(what, slabs_query, shape, th, pairs, cap, per_col, slabs):
    n, h, w = shape[:3]
    assert slabs_query == slabs, f"{what}: the planner no longer answers {slabs} slabs"
    assert cap * pairs in (256, 512)
    ntiles = -(-w // 32) * -(-h // th) * n
    per_wg = -(-ntiles // cap)
    cols = -(-ntiles // per_wg)
    assert cols * per_col == slabs, f"{what}: {ntiles} tiles in {cols} workgroup columns"
    assert cols < ntiles and per_wg >= 2, f"{what}: {ntiles} tiles on {cols} workgroup columns is no multi-item walk"
    assert ntiles < 2 * cap, f"{what}: {ntiles} tiles walk interleaved"


@functools.lru_cache(maxsize=None)      # shared by the atomics and the partials run of a case, never written
def wgrad_reference(cid):
    (n, h, w, cin, cout), (kh, kw), *_ = WGRAD_CASES[cid]
    rng = np.random.default_rng(seed(cid, 2))
    x0, bn0, x1, bn1, eff = exact_src_host(rng, n, h, w, cin, 0, True)
    dy = ints(rng, (n, cout, h, w), -2, 2) * (rng.random((n, cout, h, w)) < 0.5)
    # a priori: the sum of |x| * |dY| over the pixels of any weight element is below 2^21 (2^22 multiples of 1/2), so the fp32
    # atomics and the ordered slab sums are exact without any help from cancellation
    assert np.abs(dy).sum(axis=(0, 2, 3)).max() * np.abs(eff).max() < 2 ** 21
    dw = torch.nn.grad.conv2d_weight(t64(eff), (cout, cin, kh, kw), t64(dy), padding=pad_of(kh, kw)).numpy()
    assert np.abs(dw).max() * 2 < 2 ** 23
    return dict(src=(x0, bn0, x1, bn1), dy=dy, dw=dw)


@pytest.mark.parametrize("cid,mode", [(c, m) for c in WGRAD_CASES for m in ("atomics", "partials") if m == "atomics" or c not in ATOMICS_ONLY])
def test_wgrad_walks_bit_exact(env, cid, mode):
    """atomics mode, and partials mode (deterministic: one slab per workgroup column and row strip, summed in order by the
    unpack pass); the 7x3 launches have atomics mode only"""
    L, E = env
    shape, (kh, kw), th, pairs, cap, per_col, slabs, _ = WGRAD_CASES[cid]
    n, h, w, cin, cout = shape
    # the slab count is the walk's: queried in partials mode, for the 7x3 launches (which refuse it) with partials = 0
    d = wgrad_desc(L, shape, kh, kw, 0 if cid in ATOMICS_ONLY else 1)
    assert_wgrad_walk(cid, L.lib().oct_conv_wgrad_partials(C.byref(d)), shape, th, pairs, cap, per_col, slabs)
    if kh == 7:
        assert all(4 * b > 160 * 1024 for b in W73_STAGES.values()) and cap == 256, "a 7x3 launch may have 512 columns: one tile each"
    r = wgrad_reference(cid)
    eng = engine_for(E)
    eng.deterministic = mode == "partials"
    src = upload_src(E, cin, 0, *r["src"])
    grad = torch.full((cout, cin, kh, kw), float("nan"), dtype=torch.float32, device="cuda")
    if kh == 7:
        dwp = eng._wgrad(src, dev(r["dy"]), cout, 21, n, h, w, partials_ok=False, kh=7, kw=3)
        L.check(L.lib().oct_unpack_wgrad_kk(dwp.data_ptr(), grad.data_ptr(), cout, cin, 7, 3, 0, torch.cuda.current_stream().cuda_stream))
    else:
        dwp = eng._wgrad(src, dev(r["dy"]), cout, kh * kw, n, h, w)
        assert getattr(dwp, "_oct_nparts", 0) == (slabs if mode == "partials" else 0)
        eng._unpack(L.PACK_1X1_FPROP if kh == 1 else L.PACK_CONV_FPROP, dwp, grad, cout, cin, False)
    torch.cuda.synchronize()
    same(grad.cpu().numpy(), r["dw"], f"{cid}: wgrad ({mode})")


APPLY_STORE = (1, 152, 448)    # two 32-channel sources -> 32: 266 tiles, 2 per workgroup, DYAPPLY across both


def assert_apply_store_walk(L):
    n, h, w = APPLY_STORE
    assert L.lib().oct_conv_wgrad_apply_store_ok(C.byref(AS.desc(L, n, h, w))) == 1
    assert_wgrad_walk("apply + store", L.lib().oct_conv_wgrad_partials(C.byref(AS.desc(L, n, h, w, partials=1))),
                      APPLY_STORE, 8, 1, 256, 2, 266)


def test_wgrad_apply_store_contiguous_walk_exact_operands(env):
    """dY as stored and dW, bit for bit (the references of tests/test_gpu_wgrad_apply_store.py)"""
    assert_apply_store_walk(env[0])
    AS.test_exact_operands_give_the_same_dw_bits(env, APPLY_STORE)


def test_wgrad_apply_store_contiguous_walk_random_operands(env):
    assert_apply_store_walk(env[0])
    AS.test_dy_out_matches_the_apply_launch_and_dw_the_two_launches(env, APPLY_STORE)


# ---- first layer (first.hip): the later trips of the grid-stride loops -------------------------------------------------------------
# The planner sizes the grids by a thread per pixel and 8 channels (caps of 4096 / 512 workgroups); the kernels loop in their
# own units.  Matrix-pipe kernels (W % 32 == 0, cout >= 32): a wave per group of 32 pixels, 4 * grid groups per trip.  Direct
# stencils: a thread per pixel and 8 channels, grid * 256 / (cout / 8) pixels per trip.
# id -> ((n, h, w, cout), (kh, kw), kernel, fprop grid, fprop trips, wgrad grid, wgrad trips, smallest weight exponent, what it pins)
FIRST_CASES = {
    "f64_3x3": ((3, 112, 416, 64), (3, 3), "mfma", 4096, 1, 512, 3, -3,
                "matrix-pipe wgrad: 4368 groups on 2048 waves, three trips, the last partial (fprop: one trip, 1092 workgroups have a group)"),
    "f64_7x3": ((3, 112, 416, 64), (7, 3), "mfma", 4096, 1, 512, 3, -2, "matrix-pipe 7x3 wgrad: three trips (fprop: one)"),
    "f32_3x3_big": ((1, 592, 896, 32), (3, 3), "mfma", 4096, 2, 512, 9, -1,
                    "matrix-pipe fprop: 16576 groups on 16384 waves, a second, partial trip with the prefetched gather; wgrad: nine trips"),
    "f32_7x3_big": ((1, 592, 896, 32), (7, 3), "mfma", 4096, 2, 512, 9, -1, "matrix-pipe 7x3 fprop: second, partial trip; wgrad: nine trips"),
    "f16_direct_w": ((1, 300, 880, 16), (3, 3), "direct", 2063, 1, 512, 5, -3, "W % 32 != 0: direct stencil; wgrad: five trips (fprop: one)"),
    "f16_direct_f": ((1, 600, 880, 16), (3, 3), "direct", 4096, 2, 512, 9, -1, "direct fprop: 528000 pixels on 524288 threads' worth, a second, partial trip"),
}


def first_descs(L, cid):
    (n, h, w, cout), (kh, kw), *_ = FIRST_CASES[cid]
    k7 = (7, 3) if kh == 7 else (0, 0)
    return (L.ConvDesc(BF, n, h, w, 1, 0, cout, kh * kw, 0, 0, 0, 0, 0, 1, k7[0], k7[1], 0, 0, 0),
            L.WgradDesc(BF, n, h, w, 1, 0, cout, kh * kw, 0, 0, 0, k7[0], k7[1], 0, 0, 0, 0, 1))


def assert_first_walk(L, cid):
    """the grids are the literals of the table, and in the KERNEL's units (not the planner's) they make the loops take the
    stated number of trips"""
    (n, h, w, cout), _, kernel, gf, tf, gw, tw, _, _ = FIRST_CASES[cid]
    fd, wd = first_descs(L, cid)
    assert L.lib().oct_conv_stat_blocks(C.byref(fd)) == gf, f"{cid}: the planner no longer answers a forward grid of {gf}"
    assert L.lib().oct_conv_wgrad_partials(C.byref(wd)) == gw, f"{cid}: the planner no longer answers a wgrad grid of {gw}"
    assert kernel == ("mfma" if w % 32 == 0 and cout >= 32 else "direct")
    npix = n * h * w
    units, per_wg = (npix // 32, 4) if kernel == "mfma" else (npix, 256 // (cout // 8))
    assert -(-units // (gf * per_wg)) == tf, f"{cid}: forward, {units} units, {gf * per_wg} per trip"
    assert -(-units // (gw * per_wg)) == tw >= 2, f"{cid}: wgrad, {units} units, {gw * per_wg} per trip"
    if tf > 1:
        assert units % (gf * per_wg) != 0, f"{cid}: the last forward trip is not partial"


def first_reference(cid):
    (n, h, w, cout), (kh, kw), _, _, _, _, _, kmin, _ = FIRST_CASES[cid]
    rng = np.random.default_rng(seed(cid, 3))
    x = ints(rng, (n, 1, h, w))
    wt = pow2_weights(rng, (cout, 1, kh, kw), density=0.7, kmin=kmin)
    pad = pad_of(kh, kw)
    ref = torch.nn.functional.conv2d(t64(x), t64(wt), padding=pad).numpy()
    assert np.abs(ref).max() * 8 < 2 ** 22
    assert np.abs(ref).sum(axis=(0, 2, 3)).max() * 2.0 ** -kmin < 2 ** 24        # sum(y): below 2^24 multiples of the smallest weight
    dy = ints(rng, (n, cout, h, w), -2, 2) * (rng.random((n, cout, h, w)) < 0.5)
    assert np.abs(dy).sum(axis=(0, 2, 3)).max() * np.abs(x).max() < 2 ** 21
    dw = torch.nn.grad.conv2d_weight(t64(x), (cout, 1, kh, kw), t64(dy), padding=pad).numpy()
    assert np.abs(dw).max() * 2 < 2 ** 23
    return dict(x=x, wt=wt, ref=ref, dy=dy, dw=dw)


@pytest.mark.parametrize("cid", list(FIRST_CASES))
def test_first_layer_grid_stride_loops_bit_exact(env, cid):
    """forward with the BatchNorm sums, weight gradient in atomics and in partials mode.  The 7x3 unpack entry point takes one
    slab (the engine keeps 7x3 on atomics), so for 7x3 the test adds the slabs of partials mode itself -- exactly, by the a-priori
    bound of the reference -- before it unpacks."""
    L, E = env
    (n, h, w, cout), (kh, kw), _, gf, _, gw, _, _, _ = FIRST_CASES[cid]
    assert_first_walk(L, cid)
    r = first_reference(cid)
    eng = engine_for(E)
    src = E.Src(dev(r["x"]), 1)
    wp = packed(L, eng, fdev(r["wt"]), L.PACK_CONV_FPROP, cout, 1, kh, kw)
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    part = torch.full((gf, 2, cout), float("nan"), dtype=torch.float32, device="cuda")
    eng._conv(src, wp, cout, kh * kw, n, h, w, y, stats=part, **kk_of(kh))
    torch.cuda.synchronize()
    ref = r["ref"]
    same(host(y), to_bf16(ref), f"{cid}: first-layer fprop")
    assert not bool(torch.isnan(part).any()), f"{cid}: a row of the partial sums was not written"
    s = part.double().sum(0).cpu().numpy()
    same(s[0], ref.sum(axis=(0, 2, 3)), f"{cid}: sum(y)")
    np.testing.assert_allclose(s[1], (ref ** 2).sum(axis=(0, 2, 3)), rtol=1e-5, atol=1e-2)
    dyd = dev(r["dy"])
    for mode in ("atomics", "partials"):
        eng.deterministic = mode == "partials"
        grad = torch.full((cout, 1, kh, kw), float("nan"), dtype=torch.float32, device="cuda")
        dwp = eng._wgrad(src, dyd, cout, kh * kw, n, h, w, **kk_of(kh))
        assert getattr(dwp, "_oct_nparts", 0) == (gw if mode == "partials" else 0)
        if kh == 7:
            slab = dwp.sum(0).contiguous() if mode == "partials" else dwp
            L.check(L.lib().oct_unpack_wgrad_kk(slab.data_ptr(), grad.data_ptr(), cout, 1, 7, 3, 0, torch.cuda.current_stream().cuda_stream))
        else:
            eng._unpack(L.PACK_CONV_FPROP, dwp, grad, cout, 1, False)
        torch.cuda.synchronize()
        same(grad.cpu().numpy(), r["dw"], f"{cid}: first-layer wgrad ({mode})")


@pytest.mark.parametrize("mode", ["atomics", "partials"])
def test_first_layer_wgrad_fused_apply_later_trips_bit_exact(env, mode):
    """dy = k0 * [y*s + b > 0] * dA + k1 * y + k2 formed on load (tests/test_gpu_exact.py, same operands) where the 2048 waves
    of 512 workgroups loop over 4368 groups of 32 pixels: three trips"""
    L, E = env
    (n, h, w, f), _, _, _, _, gw, _, _, _ = FIRST_CASES["f64_3x3"]
    assert_first_walk(L, "f64_3x3")
    d = L.WgradDesc(BF, n, h, w, 1, 0, f, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1)
    assert L.lib().oct_conv_wgrad_fused_apply_ok(C.byref(d)) == 1
    rng = np.random.default_rng(seed("fused_apply"))
    x = ints(rng, (n, 1, h, w), -3, 3)
    y = ints(rng, (n, f, h, w), -4, 4)
    dA = ints(rng, (n, f, h, w), -2, 2) * (rng.random((n, f, h, w)) < 0.5)
    sc = rng.choice([-1.0, 0.5, 1.0, 2.0], f).astype(np.float32)
    sh = (rng.integers(-2, 3, f) * 0.5 + 0.25).astype(np.float32)          # never exactly zero: no tie at the mask
    coef = np.stack([rng.choice([0.5, 1.0, 2.0], f), rng.choice([-0.25, 0.0, 0.25], f), rng.choice([-0.5, 0.0, 0.5], f)]).astype(np.float32)
    bc = lambda v: v[None, :, None, None]   # noqa: E731
    mask = (y * bc(sc) + bc(sh)) > 0
    dy = bc(coef[0]) * (dA * mask) + bc(coef[1]) * y + bc(coef[2])
    assert np.array_equal(to_bf16(dy), dy)
    assert np.abs(dy).sum(axis=(0, 2, 3)).max() * np.abs(x).max() < 2 ** 21        # below 2^23 multiples of 1/4
    dw = torch.nn.grad.conv2d_weight(t64(x), (f, 1, 3, 3), t64(dy), padding=1).numpy()
    assert np.abs(dw).max() * 2 < 2 ** 23
    eng = E.UNetEngine(1, 2, 4, "bf16")
    eng.deterministic = mode == "partials"
    dwp = eng._wgrad(E.Src(dev(x), 1), dev(dA), f, 9, n, h, w, fused_apply=(dev(y), fdev(coef), fdev(sc), fdev(sh)))
    assert getattr(dwp, "_oct_nparts", 0) == (gw if mode == "partials" else 0)
    grad = torch.full((f, 1, 3, 3), float("nan"), dtype=torch.float32, device="cuda")
    eng._unpack(L.PACK_CONV_FPROP, dwp, grad, f, 1, False)
    torch.cuda.synchronize()
    same(grad.cpu().numpy(), dw, f"first-layer wgrad with fused BN-backward apply ({mode})")
