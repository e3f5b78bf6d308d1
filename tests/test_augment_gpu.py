"""ugn_assemble_modality_aug -- the training generator's random affine / mirror augmentation in the device batch assembly -- against
the numpy restatement of tests/aug_ref.py, and DataGeneratorGaitMMUWYH(augmentation_x=1, device_augmentation=True) end to end."""
import os
import random

import numpy as np
import pytest

from oracle.batch_oracle import NOISE, gaitset_layout, load_dd
from tests import aug_ref as R
from ugaitnet_amd import augment as A
from ugaitnet_amd import h5lite

pytestmark = pytest.mark.gpu

LEVEL = 1.0 / 255


def _check(got, want, levels_off, what):
    """Affine-only output: within 1e-6 of the row's largest magnitude.  Output that went through the uint8 brightness levels: >= 99.9 %
    of the elements on the identical level, the rest off by what ONE uint8 level of the normalised frame (fp32 vs the restatement's
    fp64 warp, at a truncation boundary) becomes after the brightness factor b: one level for b <= 1, one or two for b > 1
    (trunc(b q) and trunc(b (q + 1)) are up to 2 apart).  levels_off [rows]: 0 (affine only), 1 or 2."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    levels_off = np.asarray(levels_off)
    rows = got.shape[0]
    err = np.abs(got - want).reshape(rows, -1)
    tol = 1e-6 * np.abs(want).reshape(rows, -1).max(axis=1, keepdims=True)
    close = err <= tol
    k = np.rint(err / LEVEL)
    level_off = (k >= 1) & (k <= levels_off[:, None]) & (np.abs(err - k * LEVEL) <= 1e-6)
    assert (close | level_off).all(), "%s: max error %g outside the bar (rows %s)" % (
        what, err[~(close | level_off)].max(), np.nonzero(~(close | level_off).all(axis=1))[0][:8].tolist())
    photometric = levels_off > 0
    if photometric.any():
        frac = (~close[photometric]).mean()
        assert frac <= 1e-3, "%s: %.4f %% of the levels off" % (what, 100 * frac)
    return int((~close).sum())


def _levels_off(p):
    """How many brightness levels one uint8 level of a frame transformed by p can become: 0 without brightness, else 1 or 2."""
    if p is None or p.brightness is None:
        return 0
    return 1 if np.float32(p.brightness) <= 1 else 2


def _ref_base(raw, spec, aug, m, nmods):
    """aug_ref's base row of modality m of one sample: decode (with the sample's clip), transform, mirror, gaitset layout."""
    cm, cn = A.modality_clip(aug, m, nmods) if spec["compress_factor"] > 1 else (0, 0)
    seq = load_dd(raw, spec["compress_factor"], spec.get("silhouette", False), 2, cm, cn)
    p = A.modality_transform(aug, m, nmods)
    if p is not None:
        seq = R.augment_sample(seq, dict(tx=p.tx, ty=p.ty, zx=p.zx, zy=p.zy, cs=p.channel_shift, b=p.brightness), aug.flip)
    return gaitset_layout(seq)


def test_kernel_against_the_restatement(dev):
    import torch
    from ugaitnet_amd.batching import DeviceBatchAssembler, ModalitySpec
    rng = np.random.default_rng(31)
    kinds = ("of", "gray", "depth", "silhouette")
    specs = [ModalitySpec("of", 2, compress_factor=100.0), ModalitySpec("gray", 1), ModalitySpec("depth", 1), ModalitySpec("silhouette", 1)]
    ref_specs = [dict(compress_factor=100.0, channels=2), dict(compress_factor=1, channels=1), dict(compress_factor=1, channels=1),
                 dict(compress_factor=1, channels=1, silhouette=True)]
    nbase, expand = 8, 2
    raws = [rng.integers(-3000, 3000, (nbase, 60, 60, 50)).astype(np.int16), rng.integers(0, 256, (nbase, 60, 60, 25)).astype(np.uint8),
            rng.integers(0, 256, (nbase, 60, 60, 25)).astype(np.uint8),
            (rng.integers(0, 2, (nbase, 60, 60, 25)) * 255).astype(np.uint8)]
    raws[0][:, :, :, :4] = rng.integers(-40, 40, (nbase, 60, 60, 4))      # |v| < clip_min: some
    raws[0][:, :3] = 2500                                                  # |v| > clip_max: some
    for m in (1, 2, 3):                                                    # sample 5: all black
        raws[m][5] = 0
    raws[0][5] = 1234                                                      # ... with a constant optical flow
    raws[0][6] = -777
    of = lambda tx, ty, zx, zy: A.Transform(tx, ty, zx, zy)               # noqa: E731
    ph = lambda tx, ty, zx, zy, cs, b: A.Transform(tx, ty, zx, zy, cs, b)  # noqa: E731
    augs = [A.SampleAug(True, of(5, -3, 0.96, 1.04), ph(5, -3, 1.0, 1.0, 0.0, 1.0), True, A.OF_CLIP),     # OF: clip+shift+zoom+flip
            A.SampleAug(True, ph(-5, 3, 1.04, 0.9712, 0.021, 1.047), ph(0, 0, 1, 1, 0, 1), True, (0, 0)),
            A.SampleAug(True, ph(0, 5, 0.9813, 1.0277, -0.0243, 0.9531), ph(0, 0, 1, 1, 0, 1), False, A.OF_CLIP),
            A.SampleAug(False, clip=A.OF_CLIP),                                                           # randint(4) == 0
            A.SampleAug(False),
            A.SampleAug(True, ph(3, -5, 1.0113, 0.9633, 0.0131, 1.0212), ph(0, 0, 1, 1, 0, 1), True, (0, 0)),  # all black
            A.SampleAug(True, of(-3, 0, 1.0391, 0.9602), ph(0, 0, 1, 1, 0, 1), True, A.OF_CLIP),         # constant OF, affine only
            A.SampleAug(True, of(0, 0, 1.0, 1.0), ph(0, 0, 1, 1, 0, 1), False, (0, 0))]                  # the identity
    nm = len(specs)
    plan = np.full((nbase * expand, nm), -1, np.int32)
    for i in range(nbase):
        plan[i * expand] = i
        plan[i * expand + 1, ::2] = i                     # an expanded row: modalities 0 and 2 copied, 1 and 3 noise
    plan[4 * expand, 2] = -1                              # an absent modality on a base row
    asm = DeviceBatchAssembler(specs)
    out = asm.assemble(raws, plan, aug=augs)
    plain_clip = asm.assemble(raws, plan, clip=A.OF_CLIP)
    plain = asm.assemble(raws, plan)
    torch.cuda.synchronize()
    off = 0
    for m in range(nm):
        x, u = (t.cpu().numpy() for t in out[m])
        assert np.array_equal(u[:, 0], (plan[:, m] >= 0).astype(np.float32)), kinds[m]
        noise = plan[:, m] < 0
        assert (x[noise] == np.float32(NOISE)).all(), kinds[m]
        want = np.stack([_ref_base(raws[m][s], ref_specs[m], augs[s], m, nm) if s >= 0 else np.full_like(x[0], NOISE)
                         for s in plan[:, m]])
        photo = np.array([_levels_off(A.modality_transform(augs[s], m, nm)) if s >= 0 else 0 for s in plan[:, m]])
        off += _check(x, want, photo, kinds[m])
        for i in range(nbase):                            # expanded rows: the augmented base row, bit for bit
            if plan[i * expand + 1, m] >= 0 and plan[i * expand, m] == plan[i * expand + 1, m]:
                assert np.array_equal(x[i * expand + 1], x[i * expand]), (kinds[m], i)
        # untransformed samples: bit-identical to ugn_assemble_modality with the same clip
        for s, ref in ((3, plain_clip), (4, plain)):
            rows = np.nonzero(plan[:, m] == s)[0]
            assert np.array_equal(x[rows], ref[m][0].cpu().numpy()[rows]), (kinds[m], s)
        if m > 0:
            b5 = 5 * expand
            assert not x[b5].any()                        # all black through brightness: 0, not -0.5 (no range fix)
        else:
            c6 = x[6 * expand]                            # constant flow, mirrored: the x-flow planes (even t) negated
            assert np.allclose(c6[..., 0], 0.777, atol=1e-6) and np.allclose(c6[..., 1], -0.777, atol=1e-6)
            assert np.array_equal(x[7 * expand], plain[0][0].cpu().numpy()[7 * expand])     # the identity warp, unflipped
    print("elements a brightness level or two off the restatement:", off)


def _write_sample(path, data, label, gait):
    w = h5lite.Writer()
    w.create_dataset("data", data)
    for k, v in (("label", np.uint16(label)), ("videoId", np.uint16(7)), ("gait", np.uint8(gait)),
                 ("compressFactor", np.uint8(100 if data.dtype == np.int16 else 1))):
        w.set_attr("", k, v)
    w.save(path)


CONFIGS = {   # name: (nmods, dim, modality directories, expand_level)
    "3mod": (3, [(50, 60, 60), (25, 60, 60), (25, 60, 60)], ("of", "gray", "silhouette"), 3),
    "casia_b": (2, [(25, 60, 60, 2), (25, 60, 60, 1)], ("of", "gray"), 3),
    "2mod": (2, [(50, 60, 60), (25, 60, 60)], ("of", "depth"), 2),
    "1mod_gray": (1, (25, 60, 60), ("gray",), 1),
    "1mod_of": (1, (50, 60, 60), ("of",), 1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_generator_end_to_end(dev, tmp_path, name):
    from ugaitnet_amd.data.mj_dataGeneratorMMUWYHsingle_repetitions import DataGeneratorGaitMMUWYH
    nmods, dim, kinds, expand = CONFIGS[name]
    rng = np.random.default_rng(8)
    dirs = [str(tmp_path / ("%s25_60x60" % k)) for k in kinds]
    for d in dirs:
        os.makedirs(d)
    labels = [5, 5, 5, 5, 9, 9, 9, 9]
    all_samples, gaits, arrays = [], [], []
    for i, lab in enumerate(labels):
        name_i = "p%03d.h5" % i
        row = []
        for k, d in zip(kinds, dirs):
            if k == "of":
                a = rng.integers(-3000, 3000, (60, 60, 50)).astype(np.int16)
            elif k == "silhouette":
                a = (rng.integers(0, 2, (60, 60, 25)) * 255).astype(np.uint8)
            else:
                a = rng.integers(0, 256, (60, 60, 25)).astype(np.uint8)
            _write_sample(os.path.join(d, name_i), a, lab, 1)
            row.append(a)
        all_samples.append(((name_i,) * nmods, lab))
        gaits.append(1)
        arrays.append(row)
    gen = DataGeneratorGaitMMUWYH(all_samples, batch_size=8, dim=dim, n_classes=2, datadir=dirs, labmap={5: 0, 9: 1}, gait=gaits,
                                  ntype=2, augmentation_x=1, expand_level=expand, nmods=nmods, gaitset=True, repetition=2,
                                  shuffle=False, device_augmentation=True)
    withof = A.withof(dim, nmods)
    assert gen.augmentation and gen.withof == withof and withof == (name in ("3mod", "2mod", "1mod_of"))
    specs = [dict(compress_factor=100.0 if k == "of" else 1, channels=2 if k == "of" else 1, silhouette=k == "silhouette")
             for k in kinds]
    for seed in (11, 12):
        np.random.seed(seed)
        random.seed(seed)
        X, y = gen[0]                      # (one label cycle of 8 records in file order: shuffle=False, one gait type)
        want, draws = R.gen_batch(arrays, specs, nmods, withof, expand, seed, seed)
        X = [X] if nmods == 1 else X
        rows = 8 * (1 if nmods == 1 else expand)
        assert y[0].reshape(-1).tolist() == [0] * (rows // 2) + [1] * (rows // 2)
        assert sum(t is not None for t, _, _ in draws) > 0 and (withof or all(c == (0, 0) for _, _, c in draws))
        for m in range(nmods):
            base = np.arange(rows) // (rows // 8)
            k = 1 if (nmods == 2 and m == 1) else 0
            photo = np.array([0 if draws[b][0] is None or draws[b][0][k]["b"] is None else 1 + (np.float32(draws[b][0][k]["b"]) > 1)
                              for b in base])
            _check(X[2 * m if nmods > 1 else 0].cpu().numpy(), want[2 * m], photo, "%s modality %d seed %d" % (name, m, seed))
            if nmods > 1:
                assert np.array_equal(X[2 * m + 1].cpu().numpy(), want[2 * m + 1]), (name, m)
    if name != "3mod":
        return
    from ugaitnet_amd.nets.mj_uwyhNets_ba import UWYHSemiNet3Mods, optimizers, sign_max
    model = UWYHSemiNet3Mods.build_or_load([(25, 60, 60, 2), (25, 60, 60, 1), (25, 60, 60, 1)], 4, [7, 5, 3, 2],
                                           [96, 192, 512, 4096], optimizer=optimizers.Adam(lr=1e-4), nclasses=2,
                                           loss_weights=[1.0, 0.1], fMerge=sign_max, gaitset=True, seed=1)
    hist = model.fit(gen, epochs=2, steps_per_epoch=1, verbose=0)
    assert len(hist.history["loss"]) == 2 and np.isfinite(hist.history["loss"]).all()

