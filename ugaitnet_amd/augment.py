"""The training generator's random affine / mirror augmentation (`augmentation_x > 0`), host half: the parameter draws and the
records ugn_assemble_modality_aug applies on the device (ugaitnet_amd/csrc/assemble.hip).

The reference (data/mj_dataGeneratorMMUWYHsingle_repetitions.py :104-105, :392-450, :592-624, :712-742; data/mj_augmentation.py)
builds two Keras ImageDataGenerators, `mj_transgenerator(isof=withof)` and `mj_transgenerator(isof=False)`, and for every base sample
of a batch, in batch order, draws from the global np.random:
    randint(4)                  the sample is transformed iff > 0; then
        P0 = G0.get_random_transform(), P1 = G1.get_random_transform(), P1.tx, P1.ty = P0.tx, P0.ty, flip = randint(2) == 1
    randint(2) (iff withof)     == 1: the optical flow of this sample is clipped, (clip_max, clip_min) = (2300, 50)
One `get_random_transform` of these generators (keras_preprocessing 1.1.x, the tf.keras of TF 2.3) consumes, in order:
    tx = choice(SHIFTS) * choice([-1, 1]); ty likewise; zx, zy = uniform(0.96, 1.04, 2); random() twice (the horizontal / vertical
    flip decisions, both disabled); for the non-OF generator uniform(-0.025, 0.025) (channel shift) and uniform(0.95, 1.05)
    (brightness).
PARITY UNPINNED: that draw order is a reading of keras_preprocessing 1.1.x, which is not available to check against.

Which transform a modality gets follows the reference's three generators: nmods 1 -> P0; nmods 2 -> modality 0 P0, modality 1 P1;
nmods 3 -> P0 for every modality (`__gen_batchMM` applies img_gen[0] to all of them)."""
from __future__ import annotations

import numpy as np

SHIFTS = [-5, -3, 0, 3, 5]          # mj_transgenerator's `displace`, pixels
ZOOM = (0.96, 1.04)                 # zoom_range = 0.04
CHANNEL_SHIFT = 0.025               # non-OF generator only
BRIGHTNESS = (0.95, 1.05)           # non-OF generator only
OF_CLIP = (2300.0, 50.0)            # (clip_max, clip_min) of the optical-flow clipping draw
HW = 60
RECORD_WORDS = 248                  # UGN_AUG_RECORD_WORDS (include/ugaitnet_hip.h)


class Transform:
    """One `get_random_transform` of an mj_transgenerator: shift (tx rows, ty columns), zoom, and for the non-OF generator
    (photometric = True) channel shift and brightness."""

    def __init__(self, tx=0, ty=0, zx=1.0, zy=1.0, channel_shift=None, brightness=None):
        self.tx, self.ty, self.zx, self.zy = int(tx), int(ty), float(zx), float(zy)
        self.channel_shift, self.brightness = channel_shift, brightness
        if (channel_shift is None) != (brightness is None):
            raise ValueError("channel_shift and brightness come together (the non-OF generator) or not at all")

    @property
    def photometric(self):
        return self.brightness is not None

    def __repr__(self):
        return "Transform(tx=%d, ty=%d, zx=%.6f, zy=%.6f, channel_shift=%r, brightness=%r)" % (
            self.tx, self.ty, self.zx, self.zy, self.channel_shift, self.brightness)


class SampleAug:
    """What one base sample drew: transformed or not, the two transforms, the mirror, the optical-flow clip."""

    def __init__(self, transformed=False, p0=None, p1=None, flip=False, clip=(0.0, 0.0)):
        self.transformed, self.p0, self.p1, self.flip = bool(transformed), p0, p1, bool(flip)
        self.clip = (float(clip[0]), float(clip[1]))
        if self.transformed and (p0 is None or p1 is None):
            raise ValueError("a transformed sample carries both transforms")

    def __repr__(self):
        return "SampleAug(transformed=%r, p0=%r, p1=%r, flip=%r, clip=%r)" % (self.transformed, self.p0, self.p1, self.flip, self.clip)


def withof(dim, nmods):
    """The reference's literal rule (:65-68): `dim[0][0] == 50` for nmods > 1, `dim[0] == 50` for one modality.  So the legacy
    spelling (50, 60, 60) of optical flow is OF, and the gaitset spelling (25, 60, 60, 2) of the CASIA-B main is not: its optical flow
    then goes through the non-OF generator (channel shift + brightness) and never draws a clip.  Reproduced as written."""
    if nmods > 1:
        return dim[0][0] == 50
    return dim[0] == 50


def draw_transform(rng, photometric):
    # `choice(a)` of a RandomState is `a[randint(len(a))]` (uniform, with replacement, no p): the same numbers from the same state,
    # without converting the list to an array on every call (tests/test_augment.py checks both against the spelled-out sequence)
    tx = SHIFTS[rng.randint(5)]
    tx *= (-1, 1)[rng.randint(2)]
    ty = SHIFTS[rng.randint(5)]
    ty *= (-1, 1)[rng.randint(2)]
    zx, zy = rng.uniform(ZOOM[0], ZOOM[1], 2)
    rng.random()        # flip_horizontal decision (horizontal_flip=False)
    rng.random()        # flip_vertical decision (vertical_flip=False)
    if not photometric:
        return Transform(tx, ty, zx, zy)
    cs = rng.uniform(-CHANNEL_SHIFT, CHANNEL_SHIFT)
    b = rng.uniform(BRIGHTNESS[0], BRIGHTNESS[1])
    return Transform(tx, ty, zx, zy, float(cs), float(b))


def draw_sample(rng, with_of):
    if rng.randint(4) > 0:
        p0 = draw_transform(rng, photometric=not with_of)     # G0: the OF generator iff withof
        p1 = draw_transform(rng, photometric=True)            # G1: always the non-OF generator
        p1.tx, p1.ty = p0.tx, p0.ty
        aug = SampleAug(True, p0, p1, rng.randint(2) == 1)
    else:
        aug = SampleAug(False)
    if with_of and rng.randint(2) == 1:
        aug.clip = OF_CLIP
    return aug


def draw_batch(nbase, with_of, rng=np.random):
    """The draws of one batch of `nbase` base samples, in batch order, from `rng` (np.random or a np.random.RandomState)."""
    return [draw_sample(rng, with_of) for _ in range(int(nbase))]


def modality_transform(aug, m, nmods):
    """The transform modality m of this sample gets, or None."""
    if not aug.transformed:
        return None
    return aug.p1 if (nmods == 2 and m == 1) else aug.p0


def modality_clip(aug, m, nmods):
    """The two-modality generator loads its second modality without the clip (:445); the others pass it to every modality
    (it acts on int16 optical flow only)."""
    return (0.0, 0.0) if (nmods == 2 and m == 1) else aug.clip


def taps(z, shift, n=HW):
    """Row (or column) taps of the Keras affine for output lines 0..n-1: the source coordinate of line i is computed in float64 as
    scipy.ndimage.affine_transform does with Keras's matrix (offset (-z * o) + (shift + o), o = n / 2 + 0.5), clamped to [0, n-1]
    (mode 'nearest' at order 1), and split into (index, weight): value = (1 - w) f[index] + w f[min(index + 1, n - 1)].
    Weights are rounded to float32."""
    o = n / 2 + 0.5
    off = (-float(z) * o) + (float(shift) + o)
    coord = np.clip(off + float(z) * np.arange(n, dtype=np.float64), 0.0, n - 1.0)
    idx = np.floor(coord)
    w = coord - idx
    return idx.astype(np.int32), w.astype(np.float32)


def pack_records(augs, nmods, present=None, int16=None):
    """augs: one SampleAug per base sample -> int32 [nmods][nbase][RECORD_WORDS], the device records (include/ugaitnet_hip.h).
    present [nbase][nmods] bool: an absent modality is noise and is not transformed.  int16[m]: the clip acts on int16 data only."""
    nbase = len(augs)
    rec = np.zeros((nmods, nbase, RECORD_WORDS), np.int32)
    f = rec.view(np.float32)
    o = HW / 2 + 0.5
    for m in range(nmods):
        if int16 is None or int16[m]:
            f[m, :, 3:5] = [modality_clip(a, m, nmods) for a in augs]
        on = [i for i, a in enumerate(augs) if modality_transform(a, m, nmods) is not None and (present is None or present[i][m])]
        if not on:
            continue
        ps = [modality_transform(augs[i], m, nmods) for i in on]
        rec[m, on, 0] = 1
        rec[m, on, 2] = [int(augs[i].flip) for i in on]
        photo = [k for k, p in enumerate(ps) if p.photometric]
        if photo:
            rows = [on[k] for k in photo]
            rec[m, rows, 1] = 1
            f[m, rows, 5] = [ps[k].channel_shift for k in photo]
            f[m, rows, 6] = [ps[k].brightness for k in photo]
        # taps() of every transformed sample at once, rows and columns: [len(on), 2, HW]
        z = np.array([[p.zx, p.zy] for p in ps], np.float64)[:, :, None]
        t = np.array([[p.tx, p.ty] for p in ps], np.float64)[:, :, None]
        coord = np.clip(((-z * o) + (t + o)) + z * np.arange(HW, dtype=np.float64), 0.0, HW - 1.0)
        idx = np.floor(coord)
        rec[m, on, 8:68], rec[m, on, 128:188] = idx[:, 0], idx[:, 1]
        f[m, on, 68:128], f[m, on, 188:248] = (coord - idx)[:, 0], (coord - idx)[:, 1]
    return rec
