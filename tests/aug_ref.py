"""TEST INFRASTRUCTURE ONLY.  A numpy-only restatement of the training generator's random affine / mirror augmentation
(data/mj_augmentation.py and the `augmentation_x > 0` branches of data/mj_dataGeneratorMMUWYHsingle_repetitions.py), written from
the semantics of keras_preprocessing 1.1.x, scipy.ndimage and PIL -- none of which it imports: the GPU machines promise numpy and
torch only.  tests/test_augment.py checks the pieces against scipy and PIL where those are installed.

Everything works on what the reference works on: float32 frame sequences [T,60,60] as `__load_dd` returns them."""
import random

import numpy as np

from oracle.batch_oracle import NOISE, gaitset_layout, load_dd

SHIFTS = [-5, -3, 0, 3, 5]


# ---- the draws ------------------------------------------------------------------------------------------------------------
def draw_transform(photometric):
    """One ImageDataGenerator.get_random_transform of mj_transgenerator(isof=not photometric), from the global np.random."""
    tx = np.random.choice(SHIFTS) * np.random.choice([-1, 1])
    ty = np.random.choice(SHIFTS) * np.random.choice([-1, 1])
    zx, zy = np.random.uniform(0.96, 1.04, 2)
    np.random.random()
    np.random.random()
    p = dict(tx=int(tx), ty=int(ty), zx=float(zx), zy=float(zy), cs=None, b=None)
    if photometric:
        p["cs"] = np.random.uniform(-0.025, 0.025)
        p["b"] = np.random.uniform(0.95, 1.05)
    return p


def draw_sample(withof):
    """-> (trans [P0, P1] or None, flip, (clip_max, clip_min)), as `__gen_batchMM` :713-728 draws them."""
    if np.random.randint(4) > 0:
        trans = [draw_transform(not withof), draw_transform(True)]
        trans[1]["tx"], trans[1]["ty"] = trans[0]["tx"], trans[0]["ty"]
        flip = np.random.randint(2) == 1
    else:
        trans, flip = None, False
    clip = (2300, 50) if (withof and np.random.randint(2) == 1) else (0, 0)
    return trans, flip, clip


# ---- steps 1-5 ------------------------------------------------------------------------------------------------------------
def affine(frame, tx, ty, zx, zy):
    """scipy.ndimage.affine_transform(frame, Keras's matrix, order=1, mode='nearest') for a float32 frame: float64 bilinear at the
    edge-clamped source coordinates, rounded to float32."""
    n = frame.shape[0]
    o = n / 2 + 0.5

    def coords(z, t):
        c = np.clip((-z * o) + (t + o) + z * np.arange(n, dtype=np.float64), 0.0, n - 1.0)
        i0 = np.floor(c).astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1), c - i0

    r0, r1, wr = coords(zx, tx)
    c0, c1, wc = coords(zy, ty)
    f = frame.astype(np.float64)
    top = f[r0][:, c0] * (1 - wc) + f[r0][:, c1] * wc
    bot = f[r1][:, c0] * (1 - wc) + f[r1][:, c1] * wc
    return (top * (1 - wr)[:, None] + bot * wr[:, None]).astype(np.float32)


def channel_shift(frame, cs):
    """Keras apply_channel_shift on a one-channel float32 frame."""
    return np.clip(frame + np.float32(cs), frame.min(), frame.max())


def to_levels(frame):
    """Keras array_to_img(scale=True) of a one-channel float32 frame: the uint8 levels of the 'L' image."""
    x = frame.astype(np.float32)
    x = x - x.min()
    m = x.max()
    if m != 0:
        x = x / m
    x = x * np.float32(255)
    return x.astype(np.uint8)


def brightness_levels(levels, b):
    """PIL ImageEnhance.Brightness(img).enhance(b): a blend with black, alpha = (float) b, truncated (and clipped above 1)."""
    v = np.float32(b) * levels.astype(np.float32)
    return np.minimum(255, np.trunc(v)).astype(np.uint8)


def transform_frame(frame, p):
    x = affine(frame, p["tx"], p["ty"], p["zx"], p["zy"])
    if p["cs"] is not None:
        x = channel_shift(x, p["cs"])
    if p["b"] is not None:
        x = brightness_levels(to_levels(x), p["b"]).astype(np.float32)     # img_to_array: the levels, 0..255
    return x


def transform_sequence(seq, p):
    """mj_transformsequence: every frame, then the range fix (max |out| > 3 max |in| -> out / 255 - 0.5)."""
    out = np.stack([transform_frame(f, p) for f in seq])
    if float(np.abs(out).max()) > 3.0 * float(np.abs(seq).max()):
        out = out / np.float32(255.0) - np.float32(0.5)
    return out.astype(np.float32)


def mirror_sequence(seq):
    """mj_mirrorsequence: columns reversed and every EVEN plane negated, whatever the modality (`isof` is never read)."""
    out = seq[:, :, ::-1].copy()
    out[0::2] = -out[0::2]
    return out


def augment_sample(seq, p, flip):
    out = transform_sequence(seq, p)
    return mirror_sequence(out) if flip else out


# ---- the whole batch ------------------------------------------------------------------------------------------------------
def gen_batch(samples, specs, nmods, withof, expand, np_seed, py_seed):
    """The reference generator's batch with augmentation_x > 0 and gaitset=True: samples[i][m] raw `data` array or None;
    specs[m] = dict(compress_factor, silhouette, channels).  np.random is seeded with np_seed for the augmentation draws, a
    random.Random(py_seed) drives the row expansion (`__gen_batchMM` for nmods 3, `__gen_batch` for 2, none for 1).
    Returns [x0, u0, x1, u1, ...] float32 (u_m omitted for nmods 1, where X is the tensor itself) and the draws."""
    np.random.seed(np_seed)
    rng = random.Random(py_seed)
    nbase = len(samples)
    expand = 1 if nmods == 1 else max(1, expand)
    rows = nbase * expand
    x = []
    for sp in specs:
        x += [np.empty((rows, 25, 60, 60, sp["channels"]), np.float32), np.empty((rows, 1), np.float32)]
    draws = []
    for i in range(nbase):
        trans, flip, clip = draw_sample(withof)
        draws.append((trans, flip, clip))
        for m in range(nmods):
            d = samples[i][m]
            if d is None:
                x[2 * m][i * expand] = NOISE
                x[2 * m + 1][i * expand] = 0.0
                continue
            sp = specs[m]
            cm, cn = (0, 0) if (nmods == 2 and m == 1) else clip       # the 2-mod generator loads modality 1 without the clip
            seq = load_dd(d, sp["compress_factor"], sp.get("silhouette", False), 2, cm, cn)
            if trans is not None:
                seq = augment_sample(seq, trans[1] if (nmods == 2 and m == 1) else trans[0], flip)
            x[2 * m][i * expand] = gaitset_layout(seq)
            x[2 * m + 1][i * expand] = 1.0
        if nmods == 3:
            for ex in range(expand - 1):
                if i % 2 == 0:
                    ndisable = min(ex + 1, nmods - 1) if expand > 2 else rng.randrange(1, nmods, 1)
                    l_dis = [1] * nmods
                    for _ in range(ndisable):
                        l_dis[rng.randrange(0, nmods, 1)] = 0
                else:
                    l_dis = [0] * nmods
                    l_dis[(i + ex) % 3] = 1
                for j in range(nmods):
                    r = (ex + 1) + i * expand
                    if l_dis[j]:
                        x[2 * j][r], x[2 * j + 1][r] = x[2 * j][i * expand], 1.0
                    else:
                        x[2 * j][r], x[2 * j + 1][r] = NOISE, 0.0
        elif nmods == 2 and expand > 1:
            choice = rng.randrange(0, 2, 1)
            for row in range(1, expand):
                off, on = choice, 1 - choice
                r = row + i * expand
                x[2 * off][r], x[2 * off + 1][r] = NOISE, 0.0
                x[2 * on][r], x[2 * on + 1][r] = x[2 * on][i * expand], 1.0
                choice = 1 - choice
    if nmods == 1:
        x = x[:1]
    return x, draws
