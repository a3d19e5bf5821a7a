#!/usr/bin/env python3
"""Generate the NIMA fixtures under tests/golden/ from the REFERENCE's own code (build container only; needs the reference checkout).

    python tools/make_golden_nima.py --reference /path/to/UEGAN

Imports metrics/NIMA/CalcNIMA.py unmodified (torchvision is absent: empty `torchvision`, `torchvision.models` and `torchvision.transforms`
modules are injected first; CalcNIMA only touches them inside prepare_image, which is not called here -- the preparation is pinned against
Pillow directly).  No pretrained weights exist offline, so the network gets seeded random weights (uegan_amd.nima.seeded_state_dict) and
BatchNorm running statistics from ONE train-mode pass of the reference trunk over the fixture images with momentum = 1.0, which keeps the
activations in range: ReLU6 neither saturates everywhere nor dies.  Nothing of the reference is copied: the fixtures hold data only.

    nima_mbv2.npz          seed, per-tensor checksums of the seeded weights, every BatchNorm tensor, the state-dict keys with shapes and
                           dtypes, and the reference's eval-mode results (pooled 1280-vector, probabilities, mean, std per image) in fp32
                           and from a float64 copy of the reference
    nima_mbv2_images_{a,b}.npz   the synthetic 8-bit 224x224 images (smooth fields + noise of increasing strength), first and second half
    nima_mbv2_blocks.npz   outputs of blocks 1, 3, 6, 13, 17 for the first image (fp32, and the float64 copy's rounded to fp32), the large
                           early ones subsampled by a stored step, to localise a failure
    nima_mbv2_prep{0,1,2}.npz    a raw image of another size each, with Pillow's Resize(256) + CenterCrop(224) result
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import nima as N  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 20240611
N_IMAGES = 8
BLOCKS = {1: 3, 3: 2, 6: 1, 13: 1, 17: 1}          # block index -> spatial subsampling step of the stored output
PREP_SIZES = ((300, 260), (256, 400), (333, 500))   # (h, w)
MAX_BYTES = 1 << 20


def import_reference(ref):
    for name in ("torchvision", "torchvision.models", "torchvision.transforms"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, ref)
    from metrics.NIMA import CalcNIMA
    return CalcNIMA


def synthetic_image(rng, h, w, noise):
    """smooth colour field (a few low-frequency waves per channel) + uniform noise of amplitude `noise` grey levels, 8-bit"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        f = rng.uniform(0.3, 0.7)
        for _ in range(3):
            fy, fx = rng.uniform(-3, 3, 2) * 2 * np.pi
            f = f + rng.uniform(0.05, 0.2) * np.sin(fy * yy / h + fx * xx / w + rng.uniform(0, 2 * np.pi))
        img[..., c] = f
    img = img * 255.0 + rng.uniform(-noise, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def pillow_prepare(raw):
    from PIL import Image
    h, w = raw.shape[:2]
    oh, ow = N.resized_size(h, w)
    im = Image.fromarray(raw, "RGB").resize((ow, oh), Image.BILINEAR)
    top, left = int(round((oh - 224) / 2.0)), int(round((ow - 224) / 2.0))
    return np.asarray(im.crop((left, top, left + 224, top + 224)))


def run_eval(model, x, dtype):
    model = model.to(dtype).eval()
    feats = model.base_model[0]
    blocks = {}
    with torch.no_grad():
        t = x.to(dtype)
        for i in range(19):
            t = feats[i](t)
            if i in BLOCKS:
                blocks[i] = t[0].clone()
        pooled = feats[19](t).view(t.size(0), -1)
        probs = model.head(pooled.clone())
    j = torch.arange(1, 11, dtype=dtype)
    mean = (probs * j).sum(1)
    std = ((probs * (j[None] - mean[:, None]) ** 2).sum(1)).sqrt()
    return pooled, probs, mean, std, blocks


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, "%s is %d bytes" % (name, size)
    print("%-24s %7d bytes" % (name, size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    ref = import_reference(args.reference)
    torch.manual_seed(0)
    rng = np.random.default_rng(SEED + 1)
    images = np.stack([synthetic_image(rng, 224, 224, noise) for noise in np.linspace(0.0, 40.0, N_IMAGES)])
    x = torch.from_numpy(images).permute(0, 3, 1, 2).float() / 255.0

    model = ref.NIMA()
    sd = N.seeded_state_dict(SEED)
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = 1.0
    model.train()
    with torch.no_grad():
        model.base_model(x)              # running statistics := the batch statistics of the fixture images
    model.eval()
    full = model.state_dict()
    keys = list(full.keys())
    assert keys == list(N.NIMA().state_dict().keys())

    p32, q32, m32, s32, b32 = run_eval(model, x, torch.float32)
    import copy
    p64, q64, m64, s64, b64 = run_eval(copy.deepcopy(model), x, torch.float64)

    # sensitivity conditions
    assert float(m32.max() - m32.min()) >= 0.5, "mean scores span only %.3f" % float(m32.max() - m32.min())
    assert bool((p32.abs().sum(1) > 0).all()), "an all-zero pooled feature vector"
    sat = {}
    feats = model.base_model[0]
    with torch.no_grad():                # ReLU6 outputs inside the stored blocks: fraction sitting at 0 or 6
        t = x[:1]
        for i in range(18):
            if i in BLOCKS:
                u = t
                for j, layer in enumerate(feats[i].conv):
                    u = layer(u)
                    if isinstance(layer, torch.nn.ReLU6):
                        frac = float(((u == 0) | (u == 6)).float().mean())
                        sat[(i, j)] = frac
                        assert frac <= 0.9, "block %d layer %d: %.1f%% of the ReLU6 outputs at 0 or 6" % (i, j, 100 * frac)
            t = feats[i](t)
    print("mean scores", [round(v, 3) for v in m32.tolist()])
    print("ReLU6 at 0 or 6:", {k: round(v, 3) for k, v in sat.items()})
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())      # noqa: E731
    print("fp32 vs float64: pooled %.3g (rel. to max)  probs %.3g  mean %.3g  std %.3g" % (
        rel(p32, p64), float((q32.double() - q64).abs().max()), float((m32.double() - m64).abs().max()), float((s32.double() - s64).abs().max())))

    arrays = {"seed": np.array(SEED), "keys": np.array(keys), "shapes": np.array([str(tuple(full[k].shape)) for k in keys]),
              "dtypes": np.array([str(full[k].dtype) for k in keys]),
              "checksum_keys": np.array([k for k in keys if full[k].dim() == 4 or k.startswith("head.")]),
              "pooled": p32.numpy(), "probs": q32.numpy(), "mean": m32.numpy(), "std": s32.numpy(),
              "pooled64": p64.numpy(), "probs64": q64.numpy(), "mean64": m64.numpy(), "std64": s64.numpy()}
    arrays["checksums"] = np.stack([N.tensor_checksum(sd[k]) for k in arrays["checksum_keys"]])
    for k in keys:                       # every BatchNorm tensor (gamma, beta, running statistics, counter)
        if full[k].dim() <= 1 and not k.startswith("head."):
            arrays["bn/" + k] = full[k].numpy()
    save("nima_mbv2.npz", **arrays)
    half = N_IMAGES // 2                  # two files: the noisy images do not compress, and a committed file stays under 1 MiB
    save("nima_mbv2_images_a.npz", images=images[:half])
    save("nima_mbv2_images_b.npz", images=images[half:])
    blk = {"indices": np.array(sorted(BLOCKS)), "steps": np.array([BLOCKS[i] for i in sorted(BLOCKS)])}
    for i, step in BLOCKS.items():
        blk["block%d" % i] = b32[i][:, ::step, ::step].numpy()
        blk["block%d_64" % i] = b64[i][:, ::step, ::step].float().numpy()
    save("nima_mbv2_blocks.npz", **blk)
    for n, (h, w) in enumerate(PREP_SIZES):
        raw = synthetic_image(rng, h, w, 6.0 * n)
        save("nima_mbv2_prep%d.npz" % n, raw=raw, out=pillow_prepare(raw))


if __name__ == "__main__":
    main()
