"""Device-side batch assembly: time of ugn_assemble_modality for one batch, its HBM rate and the H2D
sizes of the raw and the assembled routes; then the same C3 batch (24 clips, 3 modalities) with the training generator's random
affine / mirror augmentation (ugn_assemble_modality_aug), as drawn and with every base sample transformed, beside it -- wall time
per assemble() call and the GPU time of its kernels."""
import sys, os, random
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ugaitnet_amd import augment as A
from ugaitnet_amd.batching import DeviceBatchAssembler, ModalitySpec, plan_rows

nbase, expand = 8, 3
rng = np.random.default_rng(0)
samples = [[rng.integers(-3000, 3000, (60, 60, 50)).astype(np.int16), rng.integers(0, 256, (60, 60, 25)).astype(np.uint8),
            rng.integers(0, 256, (60, 60, 25)).astype(np.uint8)] for _ in range(nbase)]
present = np.ones((nbase, 3), bool)
plan = plan_rows(present, expand, rng=random.Random(1))
raws = [torch.from_numpy(np.stack([s[j] for s in samples])).cuda() for j in range(3)]
asm = DeviceBatchAssembler([ModalitySpec("of", 2, compress_factor=100.0), ModalitySpec("gray", 1), ModalitySpec("depth", 1)])
asm.assemble(raws, plan)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    out = asm.assemble(raws, plan)
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) / 20 * 1e3
wr = sum(x.numel() * 4 for x, _ in out)
rd = sum(int((plan[:, j] >= 0).sum()) * raws[j][0].numel() * raws[j].element_size() for j in range(3))
print("GPU assembly of %d rows x 3 modalities: %.1f us (incl. 3 launches + plan upload), %.1f MB written + %.1f MB read = %.2f TB/s" % (
    plan.shape[0], us, wr / 1e6, rd / 1e6, (wr + rd) / us / 1e6))
print("H2D per batch: raw %.1f MB vs assembled float32 %.1f MB (the reference ships float64: %.1f MB)" % (
    sum(r.numel() * r.element_size() for r in raws) / 1e6, wr / 1e6, 2 * wr / 1e6))


def timed(aug, n=50):
    """(wall us per assemble() call, GPU us of its kernels alone): the second from HIP events around the C-ABI launches"""
    from ugaitnet_amd import _lib
    asm.assemble(raws, plan, aug=aug)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        asm.assemble(raws, plan, aug=aug)
    e1.record()
    torch.cuda.synchronize()
    wall = e0.elapsed_time(e1) / n * 1e3
    _lib.PROFILE = {}
    try:
        for _ in range(n):
            asm.assemble(raws, plan, aug=aug)
        torch.cuda.synchronize()
        gpu = sum(a.elapsed_time(b) for evs in _lib.PROFILE.values() for a, b in evs) / n * 1e3
    finally:
        _lib.PROFILE = None
    return wall, gpu


np.random.seed(3)
drawn = A.draw_batch(nbase, True)
every = [A.SampleAug(True, A.Transform(3, -5, 0.97, 1.03), A.Transform(3, -5, 1.01, 0.99, 0.01, 1.02), i % 2 == 0, A.OF_CLIP)
         for i in range(nbase)]
for name, aug in (("plain", None), ("augmented, as drawn (%d of %d transformed)" % (sum(a.transformed for a in drawn), nbase), drawn),
                  ("augmented, every sample transformed", every)):
    wall, gpu = timed(aug)
    print("C3 batch, %d clips x 3 modalities, %s: %.1f us per assemble() call, %.1f us GPU time of its kernels" % (
        plan.shape[0], name, wall, gpu))
