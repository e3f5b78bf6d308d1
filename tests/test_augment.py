"""The random affine / mirror augmentation's host half (ugaitnet_amd/augment.py) and the numpy restatement the GPU tests compare
against (tests/aug_ref.py): the restatement against scipy.ndimage and PIL where they are installed, the draws against a seeded
np.random, `withof` for both spellings of `dim`, the tap tables."""
import numpy as np
import pytest

from tests import aug_ref as R
from ugaitnet_amd import augment as A


def _keras_affine_scipy(frame, tx, ty, zx, zy):
    """What keras_preprocessing's apply_affine_transform does for a shift + zoom: the 3x3 matrix shift @ zoom, re-centred on
    (h / 2 + 0.5, w / 2 + 0.5), handed to scipy.ndimage.affine_transform with order 1 and mode 'nearest'."""
    ndimage = pytest.importorskip("scipy.ndimage")
    h, w = frame.shape
    m = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64) @ np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]], np.float64)
    ox, oy = h / 2 + 0.5, w / 2 + 0.5
    m = np.array([[1, 0, ox], [0, 1, oy], [0, 0, 1]]) @ m @ np.array([[1, 0, -ox], [0, 1, -oy], [0, 0, 1]])
    return ndimage.affine_transform(frame, m[:2, :2], m[:2, 2], order=1, mode="nearest", cval=0.0)


@pytest.mark.parametrize("tx,ty,zx,zy", [(0, 0, 1.0, 1.0), (5, -3, 0.96, 1.04), (-5, 5, 1.04, 0.96), (3, 0, 1.0173, 0.9712),
                                         (0, -5, 0.9861, 1.0311)])
def test_affine_matches_scipy(tx, ty, zx, zy):
    rng = np.random.default_rng(abs(tx * 7 + ty))
    for frame in (rng.standard_normal((60, 60)).astype(np.float32) * 3,
                  (rng.integers(0, 256, (60, 60)) / np.float32(255) - np.float32(0.5)).astype(np.float32)):
        want = _keras_affine_scipy(frame, tx, ty, zx, zy)
        got = R.affine(frame, tx, ty, zx, zy)
        assert want.dtype == got.dtype == np.float32
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    if (tx, ty, zx, zy) == (0, 0, 1.0, 1.0):
        assert np.array_equal(R.affine(frame, 0, 0, 1.0, 1.0), frame)


def test_brightness_levels_match_pil():
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    rng = np.random.default_rng(5)
    for b in (0.95, 0.9731, 0.999999, 1.0, 1.0000001, 1.0217, 1.05, float(np.nextafter(np.float32(1.05), np.float32(0)))):
        levels = rng.integers(0, 256, (60, 60)).astype(np.uint8)
        levels[0, :8] = [0, 1, 127, 128, 242, 243, 254, 255]
        want = np.asarray(ImageEnhance.Brightness(Image.fromarray(levels, "L")).enhance(b))
        assert np.array_equal(R.brightness_levels(levels, b), want), b


def test_array_to_img_levels():
    """Keras array_to_img(scale=True) through PIL's 'L' image: (x - min) / max * 255 truncated; a constant frame is all 0."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((60, 60)) * 0.3).astype(np.float32)
    y = x - x.min()
    y /= y.max()
    y *= 255
    want = np.asarray(Image.fromarray(y.astype("uint8"), "L"))
    assert np.array_equal(R.to_levels(x), want)
    assert not R.to_levels(np.full((60, 60), -0.5, np.float32)).any()


def test_range_fix_and_mirror_degenerate_cases():
    p = dict(tx=3, ty=-5, zx=1.01, zy=0.99, cs=0.01, b=1.02)
    black = np.full((25, 60, 60), -0.5, np.float32)               # an all-black gray recording, decoded
    assert np.array_equal(R.transform_sequence(black, p), np.zeros_like(black))          # levels 0: no range fix, stays 0
    sil = np.zeros((25, 60, 60), np.float32)
    sil[:, 20:40, 25:35] = 1.0
    out = R.transform_sequence(sil, p)
    assert out.min() == -0.5 and out.max() <= 0.5              # the range fix fires for silhouettes too: offset by -0.5
    of = np.full((50, 60, 60), 0.7, np.float32)
    q = dict(p, cs=None, b=None)
    assert np.array_equal(R.transform_sequence(of, q), of)     # affine only: never range-fixed
    m = R.mirror_sequence(np.arange(4 * 60 * 60, dtype=np.float32).reshape(4, 60, 60))
    assert m[0, 0, 0] == -59 and m[1, 0, 0] == 3600 + 59 and m[2, 0, 59] == -7200  # columns reversed, even planes negated


def _consume_documented(rng, withof):
    """The documented draw sequence of one base sample, spelled out call by call on a RandomState."""
    on = rng.randint(4) > 0
    if on:
        for photometric in (not withof, True):
            for _ in range(2):
                rng.choice([-5, -3, 0, 3, 5])
                rng.choice([-1, 1])
            rng.uniform(0.96, 1.04, 2)
            rng.random_sample()
            rng.random_sample()
            if photometric:
                rng.uniform(-0.025, 0.025)
                rng.uniform(0.95, 1.05)
        rng.randint(2)
    if withof:
        rng.randint(2)
    return on


@pytest.mark.parametrize("withof", [True, False])
def test_draws_consume_the_documented_sequence(withof):
    a, b = np.random.RandomState(77), np.random.RandomState(77)
    augs = A.draw_batch(40, withof, rng=a)
    flags = [_consume_documented(b, withof) for _ in range(40)]
    assert [g.transformed for g in augs] == flags and 15 < sum(flags) < 40
    assert a.randint(1 << 30) == b.randint(1 << 30)            # same state afterwards: nothing more, nothing less
    for g in augs:
        if g.transformed:
            assert (g.p1.tx, g.p1.ty) == (g.p0.tx, g.p0.ty) and g.p1.photometric and g.p0.photometric == (not withof)
            assert abs(g.p0.tx) in (0, 3, 5) and 0.96 <= g.p0.zx < 1.04 and 0.95 <= g.p1.brightness < 1.05
        assert g.clip in ((0.0, 0.0), (2300.0, 50.0)) and (withof or g.clip == (0.0, 0.0))
    if withof:
        assert any(g.clip == (2300.0, 50.0) for g in augs)


@pytest.mark.parametrize("withof", [True, False])
def test_draws_match_the_restatement_on_global_np_random(withof):
    np.random.seed(2024)
    augs = A.draw_batch(12, withof)
    np.random.seed(2024)
    ref = [R.draw_sample(withof) for _ in range(12)]
    for g, (trans, flip, clip) in zip(augs, ref):
        assert g.transformed == (trans is not None) and g.flip == flip and g.clip == tuple(float(c) for c in clip)
        if trans is not None:
            for p, q in ((g.p0, trans[0]), (g.p1, trans[1])):
                assert (p.tx, p.ty, p.zx, p.zy, p.channel_shift, p.brightness) == (q["tx"], q["ty"], q["zx"], q["zy"], q["cs"], q["b"])


def test_withof_follows_the_literal_rule():
    assert A.withof([(50, 60, 60), (25, 60, 60), (25, 60, 60)], 3)          # the 3-mod main
    assert not A.withof([(25, 60, 60, 2), (25, 60, 60, 1)], 2)              # the CASIA-B gaitset main: its OF is "not OF"
    assert A.withof([(50, 60, 60), (25, 60, 60)], 2)
    assert A.withof((50, 60, 60), 1) and not A.withof((25, 60, 60), 1)
    np.random.seed(3)
    augs = A.draw_batch(30, A.withof([(25, 60, 60, 2), (25, 60, 60, 1)], 2))
    assert all(g.clip == (0.0, 0.0) for g in augs)                          # no clip draw for the CASIA-B spelling
    assert all(g.p0.photometric for g in augs if g.transformed)              # and its modality 0 gets the non-OF generator


def test_tap_tables():
    idx, w = A.taps(1.0, 0)
    assert np.array_equal(idx, np.arange(60)) and not w.any()              # zoom 1, shift 0: the identity
    assert idx.dtype == np.int32 and w.dtype == np.float32
    for z in (0.96, 1.04):
        for t in (-5, 5):
            idx, w = A.taps(z, t)
            coord = np.clip(z * (np.arange(60) - 30.5) + 30.5 + t, 0, 59)
            assert idx.min() >= 0 and idx.max() <= 59 and (w >= 0).all() and (w < 1).all()
            assert np.abs(idx + w.astype(np.float64) - coord).max() < 1e-6
            if t == 5:
                assert idx[-1] == 59 and w[-1] == 0                        # clamped at the bottom edge
            else:
                assert idx[0] == 0 and w[0] == 0                           # ... and at the top


def test_records_map_transforms_to_modalities():
    p0 = A.Transform(3, -5, 0.97, 1.02)
    p1 = A.Transform(3, -5, 1.01, 0.99, 0.01, 1.03)
    augs = [A.SampleAug(True, p0, p1, True, (2300, 50)), A.SampleAug(False, clip=(2300, 50))]
    present = np.array([[True, True, False], [True, True, True]])
    r3 = A.pack_records(augs, 3, present, [True, False, False])
    f3 = r3.view(np.float32)
    assert r3.shape == (3, 2, A.RECORD_WORDS)
    assert list(r3[:, 0, 0]) == [1, 1, 0]                                   # absent modality: not transformed
    assert r3[0, 0, 1] == 0 and r3[1, 0, 1] == 0 and r3[0, 0, 2] == 1      # nmods 3: P0 (here the OF generator) everywhere
    assert tuple(f3[0, 0, 3:5]) == (2300.0, 50.0) and not f3[1, 0, 3:5].any()     # the clip acts on int16 only
    assert r3[0, 1, 0] == 0 and tuple(f3[0, 1, 3:5]) == (2300.0, 50.0)    # untransformed sample keeps its clip
    r2 = A.pack_records(augs, 2, None, [True, True])
    f2 = r2.view(np.float32)
    assert r2[0, 0, 1] == 0 and r2[1, 0, 1] == 1 and np.isclose(f2[1, 0, 6], 1.03)      # nmods 2: modality 1 gets P1
    assert not f2[1, 0, 3:5].any()                                          # ... loaded without the clip
    i, w = A.taps(1.01, 3)
    assert np.array_equal(r2[1, 0, 8:68], i) and np.array_equal(f2[1, 0, 68:128], w)


def test_refusal_names_the_keyword(tmp_path):
    """Without device_augmentation the reference's default augmentation_x=1 is still refused, and the message says how to opt in."""
    from ugaitnet_amd.data.mj_dataGeneratorMMUWYHsingle_repetitions import DataGeneratorGaitMMUWYH
    with pytest.raises(NotImplementedError, match="augmentation_x=1.*device_augmentation=True"):
        DataGeneratorGaitMMUWYH([], dim=[(50, 60, 60), (25, 60, 60)], datadir=[str(tmp_path)] * 2, gait=[], nmods=2, gaitset=True, ntype=2)
