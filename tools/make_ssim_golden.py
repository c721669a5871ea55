"""Writes tests/golden/ssim_reference.npz: the REAL reference's SSIM and L1_Charbonnier_loss (modules/losses/__init__.py, imported
through oracle/ref_stubs.py) on the inputs of tests/test_ssim.py, evaluated in float32 and in float64 (the class casts its window to
the input dtype), with autograd's gradients.  Build container only -- the reference tree is not on the GPU box.

    python tools/make_ssim_golden.py          # from the repo root

Per case <name>: <name>/shape, /window, /max_val, /seed, /x, /y (float32 inputs), /loss32, /loss64 (reduction 'none'), /d1_32, /d2_32,
/d1_64, /d2_64 (gradients of sum(loss * gmap), gmap = linspace(0.5, 1.5) over the elements), /mean64, /sum64.  Charbonnier:
charb/<name>/x, /y, /value32, /value64, /dx64, /dy64.  meta/torch = the torch version.  Numbers and key names only.

A seed is accepted only if the float64 SSIM map stays 1e-4 away from the two clamp points (|S| and |1 - S|): the gradient is
discontinuous there and a float32 evaluation may take the other branch."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "ssim_reference.npz")

# name, (B,C,H,W), window, amplitude, max_val          (tests/test_ssim.py reads the list back from the file)
CASES = [
    ("ragged", (2, 3, 37, 45), 11, 1.0, 1.0),          # ragged in both directions, several 32-tiles
    ("docstring", (1, 4, 5, 5), 5, 1.0, 1.0),          # the image is one window
    ("flat_wide", (2, 3, 9, 70), 7, 1.0, 1.0),         # less than a tile high, several wide
    ("seam", (1, 1, 33, 33), 3, 1.0, 1.0),             # one pixel past the 32-tile seam
    ("tiny", (1, 3, 3, 4), 11, 1.0, 1.0),              # image smaller than the padding
    ("window1", (1, 2, 16, 16), 1, 1.0, 1.0),          # degenerate window, sigma == 0
    ("cap", (1, 3, 20, 24), 15, 1.0, 1.0),             # the largest window with a kernel
    ("loud", (1, 3, 20, 24), 11, 2.5, 2.0),            # amplitude 2.5 against max_val 2
]
CHARB = [("small", (2, 3, 7, 9)), ("one", (1,))]
MARGIN = 1e-4


def make_inputs(shape, amplitude, seed):
    """x: a smooth field plus noise in about [-1, 1] (times amplitude); y: x plus Gaussian noise of 0.25 (times amplitude)."""
    g = torch.Generator().manual_seed(seed)
    b, c, h, w = shape
    yy = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
    xx = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    ph = torch.rand((b, c, 1, 1), generator=g, dtype=torch.float64) * 6.283185307179586
    fy = 0.15 + 0.2 * torch.rand((b, c, 1, 1), generator=g, dtype=torch.float64)
    fx = 0.15 + 0.2 * torch.rand((b, c, 1, 1), generator=g, dtype=torch.float64)
    smooth = 0.6 * torch.sin(fy * yy + ph) * torch.cos(fx * xx - ph)
    x = smooth + 0.2 * torch.randn(shape, generator=g, dtype=torch.float64)
    y = x + 0.25 * torch.randn(shape, generator=g, dtype=torch.float64)
    return (amplitude * x).float(), (amplitude * y).float()


def upstream_map(shape):
    n = int(np.prod(shape))
    return torch.linspace(0.5, 1.5, n, dtype=torch.float64).reshape(shape)


def ssim_index64(SSIM, x, y, window, max_val):
    """The float64 SSIM index itself (before the clamp), recovered through the reference's forward pieces."""
    m = SSIM(window, "none", max_val)
    c = x.shape[1]
    k = m.window.to(torch.float64).repeat(c, 1, 1, 1)
    x, y = x.double(), y.double()
    mu1, mu2 = m.filter2D(x, k, c), m.filter2D(y, k, c)
    s1 = m.filter2D(x * x, k, c) - mu1 * mu1
    s2 = m.filter2D(y * y, k, c) - mu2 * mu2
    s12 = m.filter2D(x * y, k, c) - mu1 * mu2
    return ((2 * mu1 * mu2 + m.C1) * (2 * s12 + m.C2)) / ((mu1 * mu1 + mu2 * mu2 + m.C1) * (s1 + s2 + m.C2))


def evaluate(SSIM, x, y, window, max_val, gmap, dtype):
    a = x.detach().to(dtype).clone().requires_grad_(True)
    b = y.detach().to(dtype).clone().requires_grad_(True)
    loss = SSIM(window, "none", max_val)(a, b)
    (loss * gmap.to(dtype)).sum().backward()
    return loss.detach(), a.grad, b.grad


def main():
    from oracle import ref_stubs
    ref_stubs.install()
    from modules.losses import SSIM, L1_Charbonnier_loss          # the reference's own
    assert sys.modules["modules.losses"].__file__.startswith(ref_stubs.REFERENCE_ROOT)
    out = {"meta/torch": np.array(torch.__version__), "meta/cases": np.array([c[0] for c in CASES]),
           "meta/charb": np.array([c[0] for c in CHARB])}
    for idx, (name, shape, window, amplitude, max_val) in enumerate(CASES):
        for seed in range(100000 * idx + 1, 100000 * idx + 50000):
            x, y = make_inputs(shape, amplitude, seed)
            S = ssim_index64(SSIM, x, y, window, max_val)
            if float(S.abs().min()) >= MARGIN and float((1 - S).abs().min()) >= MARGIN:
                break
        else:
            raise SystemExit("no seed keeps case %s away from the clamp points" % name)
        gmap = upstream_map(shape)
        l32, a32, b32 = evaluate(SSIM, x, y, window, max_val, gmap, torch.float32)
        l64, a64, b64 = evaluate(SSIM, x, y, window, max_val, gmap, torch.float64)
        print("%-10s seed %5d  S in [%.3f, %.3f]  clamped %d / %d  float32 vs float64: map %.2e  d1 %.2e  d2 %.2e" % (
            name, seed, float(S.min()), float(S.max()), int((S < 0).sum()), S.numel(),
            float((l32.double() - l64).norm() / l64.norm()), float((a32.double() - a64).norm() / a64.norm()),
            float((b32.double() - b64).norm() / b64.norm())))
        p = name + "/"
        out[p + "shape"], out[p + "window"], out[p + "max_val"], out[p + "seed"] = np.array(shape), np.array(window), np.array(max_val), np.array(seed)
        out[p + "x"], out[p + "y"] = x.numpy(), y.numpy()
        out[p + "loss32"], out[p + "d1_32"], out[p + "d2_32"] = l32.numpy(), a32.numpy(), b32.numpy()
        out[p + "loss64"], out[p + "d1_64"], out[p + "d2_64"] = l64.numpy(), a64.numpy(), b64.numpy()
        out[p + "mean64"] = SSIM(window, "mean", max_val)(x.double(), y.double()).numpy()
        out[p + "sum64"] = SSIM(window, "sum", max_val)(x.double(), y.double()).numpy()
    crit = L1_Charbonnier_loss()
    for idx, (name, shape) in enumerate(CHARB):
        g = torch.Generator().manual_seed(9000 + idx)
        x = torch.randn(shape, generator=g)
        y = x + 0.25 * torch.randn(shape, generator=g)
        p = "charb/" + name + "/"
        out[p + "x"], out[p + "y"] = x.numpy(), y.numpy()
        out[p + "value32"] = crit(x, y).numpy()
        a, b = x.double().requires_grad_(True), y.double().requires_grad_(True)
        v = crit(a, b)
        v.backward()
        out[p + "value64"], out[p + "dx64"], out[p + "dy64"] = v.detach().numpy(), a.grad.numpy(), b.grad.numpy()
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
