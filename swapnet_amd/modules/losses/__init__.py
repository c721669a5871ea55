"""modules.losses of the reference (its modules/losses/__init__.py): PerceptualLoss (perceptual.py, the texture stage's
content / style terms), SSIM / ssim, L1_Charbonnier_loss and the Gaussian window helpers.  (GANLoss is modules.loss.GANLoss.)

SSIM and L1_Charbonnier_loss on CUDA float32 tensors run as fused HIP kernels (csrc/ssim.hip through engine.op_ssim /
op_charbonnier on engine.default_context()), forward and backward; any other input (CPU tensors, float64) evaluates the same
formula with torch ops and torch's autograd."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from ... import engine
from .perceptual import PerceptualLoss  # noqa: F401

__all__ = ["PerceptualLoss", "SSIM", "ssim", "L1_Charbonnier_loss", "gaussian", "get_gaussian_kernel1d", "get_gaussian_kernel2d"]


def gaussian(window_size, sigma):
    """Normalised float32 Gaussian of `window_size` taps centred on the window (half a tap off centre for an even size)."""
    x = torch.arange(window_size).float() - window_size // 2
    if window_size % 2 == 0:
        x = x + 0.5
    g = torch.exp(-x.pow(2.0) / float(2 * sigma ** 2))
    return g / g.sum()


def get_gaussian_kernel1d(kernel_size, sigma, force_even=False):
    """(kernel_size,) Gaussian filter coefficients; TypeError unless kernel_size is a positive int, odd unless force_even."""
    if not isinstance(kernel_size, int) or kernel_size <= 0 or (kernel_size % 2 == 0 and not force_even):
        raise TypeError("kernel_size must be an odd positive integer. Got {}".format(kernel_size))
    return gaussian(kernel_size, sigma)


def get_gaussian_kernel2d(kernel_size, sigma, force_even=False):
    """(kx, ky) matrix of Gaussian coefficients: the outer product of the two 1-D kernels."""
    if not isinstance(kernel_size, tuple) or len(kernel_size) != 2:
        raise TypeError("kernel_size must be a tuple of length two. Got {}".format(kernel_size))
    if not isinstance(sigma, tuple) or len(sigma) != 2:
        raise TypeError("sigma must be a tuple of length two. Got {}".format(sigma))
    kx = get_gaussian_kernel1d(kernel_size[0], sigma[0], force_even)
    ky = get_gaussian_kernel1d(kernel_size[1], sigma[1], force_even)
    return torch.matmul(kx.unsqueeze(-1), ky.unsqueeze(-1).t())


def _native(t):
    return t.is_cuda and t.dtype == torch.float32


def _context_of(t):
    """The process's default context when the tensor lives on the current device (the one PerceptualLoss uses), else that device's."""
    return engine.default_context(None if t.device.index == torch.cuda.current_device() else t.device.index)


class _SsimFn(torch.autograd.Function):
    """(loss map | sum | mean) of swn_op_ssim; backward = the same call with the upstream gradient, both image gradients at once."""

    @staticmethod
    def forward(fctx, img1, img2, window, max_val, reduction):
        ctx = _context_of(img1)
        a, b = img1.detach().contiguous(), img2.detach().contiguous()
        total, lmap, _, _ = engine.op_ssim(ctx, a, b, window, max_val, want_map=reduction == "none")
        fctx.save_for_backward(a, b)
        fctx.cfg = (ctx, window, max_val, reduction)
        if reduction == "none":
            return lmap
        return total[0] / a.numel() if reduction == "mean" else total[0].clone()

    @staticmethod
    @once_differentiable
    def backward(fctx, g):
        a, b = fctx.saved_tensors
        ctx, window, max_val, reduction = fctx.cfg
        if reduction == "none":
            up = g.contiguous()
        else:
            up = float(g) / a.numel() if reduction == "mean" else float(g)
        _, _, d1, d2 = engine.op_ssim(ctx, a, b, window, max_val, grad=up, want_grad=tuple(fctx.needs_input_grad[:2]))
        return d1, d2, None, None, None


class _CharbonnierFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, x, y, eps):
        ctx = _context_of(x)
        a, b = x.detach().contiguous(), y.detach().contiguous()
        total, _, _ = engine.op_charbonnier(ctx, a, b, eps)
        fctx.save_for_backward(a, b)
        fctx.cfg = (ctx, eps, x.shape, y.shape)
        return total[0].clone()

    @staticmethod
    @once_differentiable
    def backward(fctx, g):
        a, b = fctx.saved_tensors
        ctx, eps, xs, ys = fctx.cfg
        _, dx, dy = engine.op_charbonnier(ctx, a, b, eps, grad=float(g), want_grad=tuple(fctx.needs_input_grad[:2]))
        return (dx.reshape(xs) if dx is not None else None), (dy.reshape(ys) if dy is not None else None), None


class L1_Charbonnier_loss(nn.Module):
    """sum(sqrt((X - Y)^2 + eps)), eps = 1e-6."""

    def __init__(self):
        super().__init__()
        self.eps = 1e-6

    def forward(self, X, Y):
        if torch.is_tensor(X) and torch.is_tensor(Y) and _native(X) and _native(Y) and X.shape == Y.shape and X.numel() > 0:
            return _CharbonnierFn.apply(X, Y, self.eps)
        diff = torch.add(X, -Y)
        return torch.sum(torch.sqrt(diff * diff + self.eps))


class SSIM(nn.Module):
    """Structural dissimilarity (1 - SSIM) / 2 between two (B,C,H,W) images under a window_size x window_size Gaussian of sigma 1.5,
    zero padded, per channel; reduction 'none' | 'mean' | 'sum'; max_val = the dynamic range of the images."""

    def __init__(self, window_size, reduction="none", max_val=1.0):
        super().__init__()
        self.window_size = window_size
        self.max_val = max_val
        self.reduction = reduction
        self.window = get_gaussian_kernel2d((window_size, window_size), (1.5, 1.5))
        self.padding = self.compute_zero_padding(window_size)
        self.C1 = (0.01 * self.max_val) ** 2
        self.C2 = (0.03 * self.max_val) ** 2

    @staticmethod
    def compute_zero_padding(kernel_size):
        return (kernel_size - 1) // 2

    def filter2D(self, input, kernel, channel):
        return F.conv2d(input, kernel, padding=self.padding, groups=channel)

    def _torch_forward(self, img1, img2):
        """The formula with torch ops (CPU tensors, float64): five depthwise convolutions and the element-wise passes."""
        c = img1.shape[1]
        kernel = self.window.to(img1.device).to(img1.dtype).repeat(c, 1, 1, 1)
        mu1, mu2 = self.filter2D(img1, kernel, c), self.filter2D(img2, kernel, c)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        sigma1_sq = self.filter2D(img1 * img1, kernel, c) - mu1_sq
        sigma2_sq = self.filter2D(img2 * img2, kernel, c) - mu2_sq
        sigma12 = self.filter2D(img1 * img2, kernel, c) - mu1_mu2
        ssim_map = ((2 * mu1_mu2 + self.C1) * (2 * sigma12 + self.C2)) / ((mu1_sq + mu2_sq + self.C1) * (sigma1_sq + sigma2_sq + self.C2))
        loss = torch.clamp(1.0 - ssim_map, min=0, max=1) / 2.0
        if self.reduction == "mean":
            return torch.mean(loss)
        if self.reduction == "sum":
            return torch.sum(loss)
        return loss

    def forward(self, img1, img2):
        if not torch.is_tensor(img1):
            raise TypeError("Input img1 type is not a torch.Tensor. Got {}".format(type(img1)))
        if not torch.is_tensor(img2):
            raise TypeError("Input img2 type is not a torch.Tensor. Got {}".format(type(img2)))
        if len(img1.shape) != 4:
            raise ValueError("Invalid img1 shape, we expect BxCxHxW. Got: {}".format(img1.shape))
        if len(img2.shape) != 4:
            raise ValueError("Invalid img2 shape, we expect BxCxHxW. Got: {}".format(img2.shape))
        if img1.shape != img2.shape:
            raise ValueError("img1 and img2 shapes must be the same. Got: {} and {}".format(img1.shape, img2.shape))
        if img1.device != img2.device:
            raise ValueError("img1 and img2 must be in the same device. Got: {} and {}".format(img1.device, img2.device))
        if img1.dtype != img2.dtype:
            raise ValueError("img1 and img2 must be in the same dtype. Got: {} and {}".format(img1.dtype, img2.dtype))
        if _native(img1) and img1.numel() > 0:
            if self.window_size > engine.SSIM_MAX_WINDOW:
                raise NotImplementedError("SSIM on the device: windows larger than %d are not implemented, got %d"
                                          % (engine.SSIM_MAX_WINDOW, self.window_size))
            reduction = self.reduction if self.reduction in ("mean", "sum") else "none"       # (anything else reduces nothing)
            return _SsimFn.apply(img1, img2, self.window_size, float(self.max_val), reduction)
        return self._torch_forward(img1, img2)


def ssim(img1, img2, window_size, reduction="none", max_val=1.0):
    """Functional form of SSIM."""
    return SSIM(window_size, reduction, max_val)(img1, img2)
