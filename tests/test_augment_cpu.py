"""CPU: the augmentation's generator, parameter builders, draws and argument checks, and the numpy restatement itself against
plain numpy operations.  No GPU: nothing here launches a kernel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import augment_ref as R
from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
from retinal_oct_image_segmentation_via_deep_learning_amd import augment as A

ONE = 1 << 24
# Philox4x32-10 known answers (counter, key, words)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("gen", [R.philox, A.philox4x32_10], ids=["restatement", "product"])
def test_philox_known_answers(gen):
    for ctr, key, want in KAT:
        got = gen(np.array([ctr], dtype=np.uint64), key)
        assert got.dtype == np.uint32 and [int(v) for v in got[0]] == list(want), [hex(int(v)) for v in got[0]]


def test_product_generator_equals_restatement_on_many_counters():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(4096, 4), dtype=np.uint64)
    assert np.array_equal(A.philox4x32_10(ctr, (123, 456)), R.philox(ctr, (123, 456)))


def test_identity_flip_and_quarter_turn_coefficients_are_exact():
    p = A.AugmentParams.identity(3, (29, 41))
    assert p.matrix.dtype == np.int64 and p.matrix.tolist() == [[ONE, 0, 0, 0, ONE, 0]] * 3
    assert p.flags == 0 and p.intensity[0].tolist() == [1, 0, 1, 0, 0, -np.inf, np.inf]
    # a centred window on whole pixels: the difference of the sizes is odd in both directions here
    assert A.AugmentParams.identity(1, (29, 41), (24, 36)).matrix.tolist() == [[ONE, 0, 2 * ONE, 0, ONE, 2 * ONE]]
    assert A.AugmentParams.hflip(1, (29, 41)).matrix.tolist() == [[-ONE, 0, 40 * ONE, 0, ONE, 0]]
    assert A.AugmentParams.vflip(1, (29, 41)).matrix.tolist() == [[ONE, 0, 0, 0, -ONE, 28 * ONE]]
    # 90 degrees, (16, 24) -> (24, 16): cos quantises to 0, the offsets are whole pixels
    q = A.AugmentParams.compose(1, (16, 24), (24, 16), rotate_deg=90.0)
    assert q.matrix.tolist() == [[0, -ONE, 23 * ONE, ONE, 0, 0]]
    # round-half-even, once: 2^-25 is half a unit of Q24
    m = np.array([[[1 + 2.0 ** -25, 3 * 2.0 ** -25, 0], [0, 1, -2.0 ** -25]]])
    assert A.AugmentParams.from_matrices(m, (8, 8), (8, 8)).matrix.tolist() == [[ONE, 2, 0, 0, ONE, 0]]
    w = A.AugmentParams.hflip(2, (29, 41)).words()
    assert w.shape == (2, 16) and w.dtype == np.uint32
    assert w[0, :8].tolist() == [0xFF000000, 0, 0, ONE, (40 * ONE) & 0xFFFFFFFF, (40 * ONE) >> 32, 0, 0]
    assert w[0, 8:15].view(np.float32).tolist() == [1, 0, 1, 0, 0, -np.inf, np.inf]


@pytest.fixture(scope="module")
def sample():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, size=(2, 3, 16, 24), dtype=np.uint8)
    target = rng.integers(0, 9, size=(2, 16, 24), dtype=np.uint8)
    mask = rng.integers(0, 2, size=(2, 2, 16, 24), dtype=np.uint8)
    weight = rng.random((2, 16, 24), dtype=np.float32)
    return src, target, mask, weight


def _ref(sample, p, **kw):
    src, target, mask, weight = sample
    return R.augment(src, p.matrix, p.out_hw, p.intensity, p.gamma, p.noise, p.disp, p.pitch, target=target, mask=mask,
                     weight=weight, **kw)


def test_restatement_identity_flip_shift_and_quarter_turn(sample):
    src, target, mask, weight = sample
    o = _ref(sample, A.AugmentParams.identity(2, (16, 24)))
    assert np.array_equal(o["image"], src.astype(np.float32)) and np.array_equal(o["target"], target.astype(np.int64))
    assert np.array_equal(o["mask"], mask) and np.array_equal(o["weight"], weight)
    o = _ref(sample, A.AugmentParams.hflip(2, (16, 24)))
    assert np.array_equal(o["image"], np.flip(src, -1).astype(np.float32)) and np.array_equal(o["target"], np.flip(target, -1))
    assert np.array_equal(o["mask"], np.flip(mask, -1)) and np.array_equal(o["weight"], np.flip(weight, -1))
    o = _ref(sample, A.AugmentParams.vflip(2, (16, 24)))
    assert np.array_equal(o["image"], np.flip(src, -2).astype(np.float32)) and np.array_equal(o["weight"], np.flip(weight, -2))
    # content moves 3 right and 2 up; what comes in from outside reads fill / label_fill / 0
    o = _ref(sample, A.AugmentParams.compose(2, (16, 24), translate=(3, -2)), fill=7.0, label_fill=255)

    def shifted(a, outside):
        s = np.full_like(a, outside)
        s[..., :-2, 3:] = a[..., 2:, :-3]
        return s
    assert np.array_equal(o["image"], shifted(src.astype(np.float32), 7.0))
    assert np.array_equal(o["target"], shifted(target.astype(np.int64), 255)) and np.array_equal(o["mask"], shifted(mask, 255))
    assert np.array_equal(o["weight"], shifted(weight, 0.0))
    o = _ref(sample, A.AugmentParams.compose(2, (16, 24), (24, 16), rotate_deg=90.0))
    assert np.array_equal(o["image"], np.rot90(src, 1, (-2, -1)).astype(np.float32))
    assert np.array_equal(o["target"], np.rot90(target, 1, (-2, -1))) and np.array_equal(o["weight"], np.rot90(weight, 1, (-2, -1)))
    o = _ref(sample, A.AugmentParams.compose(2, (16, 24), (24, 16), rotate_deg=-90.0))
    assert np.array_equal(o["image"], np.rot90(src, -1, (-2, -1)).astype(np.float32))


def test_restatement_elastic_blend_is_the_plain_bilinear_of_the_nodes():
    """with every node the same the field is that constant; a ramp of nodes blends to the exact ramp"""
    out_hw, pitch = (19, 37), 8
    gh, gw = R.grid_shape(out_hw, pitch)
    assert (gh, gw) == (4, 6) == A.grid_shape(out_hw, pitch)
    const = np.full((gh, gw), -5 * ONE - 3, dtype=np.int32)
    assert (R.displacement(const, out_hw, pitch) == -5 * ONE - 3).all()
    ramp = (np.arange(gw, dtype=np.int32) * pitch * 1000)[None, :].repeat(gh, 0)
    assert np.array_equal(R.displacement(ramp, out_hw, pitch), np.arange(37, dtype=np.int64)[None, :].repeat(19, 0) * 1000)


def test_draws_depend_on_seed_step_and_global_index_only():
    kw = dict(hflip=0.5, vflip=0.3, rotate_deg=15, scale=(0.8, 1.25), translate=(0.1, 0.05), elastic_pitch=8, elastic_sigma_px=3.0,
              gain=(0.9, 1.1), bias=(-0.05, 0.05), gamma=(0.7, 1.5), speckle=0.1, noise=0.02, seed=0x1234567890ABCDEF)
    whole = A.PairAugmenter(**kw).draw(8, (40, 56), step=5)
    again = A.PairAugmenter(**kw).draw(8, (40, 56), step=5)
    assert np.array_equal(whole.matrix, again.matrix) and np.array_equal(whole.disp, again.disp)
    # two ranks of 4, and batches of 2 at their bases
    for rank in (0, 1):
        part = A.PairAugmenter(rank=rank, **kw).draw(4, (40, 56), step=5)
        sl = slice(4 * rank, 4 * rank + 4)
        assert np.array_equal(part.matrix, whole.matrix[sl]) and np.array_equal(part.intensity, whole.intensity[sl])
        assert np.array_equal(part.disp, whole.disp[sl])
    part = A.PairAugmenter(**kw).draw(2, (40, 56), step=5, sample_base=6)
    assert np.array_equal(part.matrix, whole.matrix[6:]) and np.array_equal(part.disp, whole.disp[6:])
    other = A.PairAugmenter(**kw).draw(8, (40, 56), step=6)
    assert not np.array_equal(other.matrix, whole.matrix) and not np.array_equal(other.disp, whole.disp)
    kw["seed"] = 1
    assert not np.array_equal(A.PairAugmenter(**kw).draw(8, (40, 56), step=5).matrix, whole.matrix)


def test_draws_respect_their_ranges():
    aug = A.PairAugmenter(hflip=0.5, rotate_deg=20, scale=(0.8, 1.25), translate=(0.1, 0.2), elastic_pitch=16, elastic_sigma_px=30.0,
                          gain=(0.9, 1.1), bias=(-0.05, 0.05), gamma=(0.7, 1.5), speckle=0.1, noise=0.02, clamp=(0.0, 1.0), seed=3)
    p = aug.draw(256, (64, 96))
    m = p.matrix.astype(np.float64) / ONE
    det = m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3]            # +-1 / scale^2
    assert (np.abs(det) >= 1 / 1.25 ** 2 - 1e-6).all() and (np.abs(det) <= 1 / 0.8 ** 2 + 1e-6).all()
    flipped = det < 0
    assert 0.3 < flipped.mean() < 0.7
    ang = np.degrees(np.arctan2(m[:, 3], m[:, 4]))          # d = sin / s, e = cos / s: vflip is off
    assert (np.abs(ang) <= 20 + 1e-4).all() and ang.std() > 5
    it = p.intensity
    assert (it[:, 0] >= 0.9).all() and (it[:, 0] <= 1.1).all() and (np.abs(it[:, 1]) <= 0.05).all()
    assert (it[:, 2] >= 0.7).all() and (it[:, 2] <= 1.5).all() and it[:, 2].std() > 0.1
    assert (it[:, 3] == np.float32(0.1)).all() and (it[:, 4] == np.float32(0.02)).all()
    assert (it[:, 5] == 0).all() and (it[:, 6] == 1).all() and p.gamma and p.noise
    assert p.disp.shape == (256, 2, 5, 7) and np.abs(p.disp).max() == 64 * ONE      # 3 sigma = 90 px: cut at 64
    # the window centre moves by at most the translate fraction (in source pixels: the output shift through the matrix)
    centre = np.stack([m[:, 0] * 47.5 + m[:, 1] * 31.5 + m[:, 2] - 47.5, m[:, 3] * 47.5 + m[:, 4] * 31.5 + m[:, 5] - 31.5], -1)
    assert (np.hypot(centre[:, 0], centre[:, 1]) <= np.hypot(0.1 * 96, 0.2 * 64) * 1.25 + 1e-3).all()
    plain = A.PairAugmenter().draw(4, (8, 8))
    assert plain.matrix.tolist() == [[ONE, 0, 0, 0, ONE, 0]] * 4 and plain.flags == 0 and plain.disp is None


def test_state_dict_round_trip():
    aug = A.PairAugmenter(seed=7, rank=2)
    aug.step = 41
    assert aug.state_dict() == {"seed": 7, "step": 41}
    other = A.PairAugmenter()
    other.load_state_dict(aug.state_dict())
    assert (other.seed, other.step) == (7, 41)
    with pytest.raises(ValueError):
        other.load_state_dict({"seed": -1, "step": 0})


def test_argument_validation():
    P = A.AugmentParams
    with pytest.raises(ValueError, match="not accepted by the geometry"):
        A.PairAugmenter(out_size=(8193, 16))
    with pytest.raises(ValueError, match="not accepted by the geometry"):
        P.identity(1, (16, 16), (0, 4))
    with pytest.raises(ValueError, match="not accepted by the geometry"):
        P.from_matrices(np.array([[[8.0, 0, 0], [0, 1, 0]]]), (16, 16), (16, 16))
    with pytest.raises(ValueError, match="power of two"):
        A.PairAugmenter(elastic_pitch=12, elastic_sigma_px=1.0)
    with pytest.raises(ValueError, match="needs elastic_pitch"):
        A.PairAugmenter(elastic_sigma_px=1.0)
    with pytest.raises(ValueError, match="probability"):
        A.PairAugmenter(hflip=1.5)
    with pytest.raises(ValueError):
        A.PairAugmenter(scale=(1.2, 0.8))
    with pytest.raises(ValueError):
        A.PairAugmenter(gamma=(0.0, 1.0))
    with pytest.raises(L.OctError, match="out_dtype"):
        A.PairAugmenter(out_dtype=torch.float16)
    with pytest.raises(TypeError, match="label_fill"):
        A.PairAugmenter(label_fill=1.5)
    with pytest.raises(ValueError, match="disp must be int32"):
        P.identity(1, (16, 16)).with_displacement(np.zeros((1, 2, 3, 4), dtype=np.int32), 8)
    with pytest.raises(ValueError, match="at most 64"):
        P.identity(1, (16, 16)).with_displacement(np.full((1, 2, 3, 3), 65 * ONE, dtype=np.int32), 8)
    aug = A.PairAugmenter()
    with pytest.raises(L.OctError, match="no CPU fallback"):
        aug(torch.zeros(1, 1, 8, 8))
    with pytest.raises(L.OctError, match="no CPU fallback"):
        A.augment_pair(torch.zeros(1, 1, 8, 8), P.identity(1, (8, 8)))
    with pytest.raises(TypeError, match="torch tensor"):
        aug(np.zeros((1, 1, 8, 8), dtype=np.float32))
    assert aug.step == 0   # a refused call does not advance the step


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.lib()


def _desc(**kw):
    v = dict(batch=1, cin=1, hs=8, ws=8, ho=8, wo=8, src_elem=L.AUG_U8, out_elem=L.AUG_BF16, label_kind=L.AUG_LABEL_NONE,
             label_planes=0, flags=0, grid_pitch=0, seed_lo=0, seed_hi=0, step=0, sample_base=0, fill=0.0, reserved=0, label_fill=0)
    v.update(kw)
    return L.AugmentDesc(**v)


def test_library_rejects_bad_descriptors_without_a_gpu(lib):
    """host-side validation comes before any launch: every call below returns -22 with nothing enqueued"""
    buf = (C.c_uint64 * 64)()      # host memory standing in for the device pointers: validation never reads it
    p = C.addressof(buf)

    def call(d, src=p, labels=None, weight=None, params=p, disp=None, out=p, labels_out=None, weight_out=None):
        return lib.oct_augment_pair(C.byref(d) if d is not None else None, src, labels, weight, params, disp, out, labels_out,
                                    weight_out, None)
    assert call(None) == -22 and "null descriptor" in L.last_error()
    assert call(_desc(ws=8193)) == -22 and "8192" in L.last_error()
    assert call(_desc(ho=0)) == -22
    assert call(_desc(src_elem=3)) == -22 and "source" in L.last_error()
    assert call(_desc(out_elem=L.AUG_U8)) == -22 and "output" in L.last_error()
    assert call(_desc(label_kind=4)) == -22 and "label kind" in L.last_error()
    assert call(_desc(flags=8)) == -22 and "flags" in L.last_error()
    assert call(_desc(flags=L.AUG_ELASTIC, grid_pitch=12), disp=p) == -22 and "power of two" in L.last_error()
    assert call(_desc(flags=L.AUG_ELASTIC, grid_pitch=0), disp=p) == -22
    assert call(_desc(flags=L.AUG_ELASTIC, grid_pitch=8)) == -22 and "displacement" in L.last_error()
    assert call(_desc(), src=None) == -22 and "null image" in L.last_error()
    assert call(_desc(), out=None) == -22
    assert call(_desc(), params=None) == -22 and "null params" in L.last_error()
    assert call(_desc(label_kind=L.AUG_LABEL_CLASS_U8)) == -22 and "null labels" in L.last_error()
    assert call(_desc(label_kind=L.AUG_LABEL_MASK_U8, label_planes=0), labels=p, labels_out=p) == -22
    assert call(_desc(label_kind=L.AUG_LABEL_MASK_U8, label_planes=1, label_fill=256), labels=p, labels_out=p) == -22
    assert call(_desc(), weight=p) == -22 and "go together" in L.last_error()
    assert call(_desc(fill=float("nan"))) == -22 and "finite" in L.last_error()
    assert call(_desc(out_elem=L.AUG_F32), out=p + 2) == -22 and "aligned" in L.last_error()
    assert call(_desc(batch=0)) == 0      # an empty batch is not an error and launches nothing
    assert lib.oct_augment_philox_words(None, 4, 0, 0, None, None) == -22 and "null pointer" in L.last_error()
    assert lib.oct_augment_philox_words(None, 0, 0, 0, None, None) == 0
