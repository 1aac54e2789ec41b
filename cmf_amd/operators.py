"""Dense measurement operators for ``ManifoldProjector.recover(..., space="data")``, built on the host: float32
(M, D) matrices that act on an input of ``shape`` = (C, H, W) flattened as ``x.flatten(1)``, so that ``x.flatten(1) @ A.T`` is the
measurement.

    A = cmf_amd.downsample((1, 28, 28), 2) @ cmf_amd.blur((1, 28, 28), torch.full((3, 3), 1 / 9))     # (196, 784), on the CPU
    out = proj.recover((x.flatten(1) @ A.T).cuda(), A.cuda(), x_init=x0.cuda(), space="data")

The matrices are dense because the operator kernel is: at D = 784 a blur holds 784^2 floats of which 9 per row are not zero."""
import torch

__all__ = ["blur", "downsample"]


def _chw(shape):
    if len(shape) != 3 or any(int(n) < 1 for n in shape):
        raise ValueError(f"shape must be (C, H, W) with positive sizes, got {tuple(shape)}")
    return tuple(int(n) for n in shape)


def blur(shape, kernel):
    """The (D, D) float32 matrix, D = C H W, of the 2-D correlation of every channel with ``kernel`` (kh, kw), kh and kw odd, under
    zero padding at "same" size: what ``torch.nn.functional.conv2d(x, kernel[None, None], padding=(kh // 2, kw // 2))`` does to
    each channel of x."""
    C, H, W = _chw(shape)
    kernel = torch.as_tensor(kernel, dtype=torch.float32)
    if kernel.dim() != 2 or kernel.shape[0] % 2 == 0 or kernel.shape[1] % 2 == 0:
        raise ValueError(f"kernel must be (kh, kw) with odd kh and kw, got {tuple(kernel.shape)}")
    kh, kw = kernel.shape
    a = torch.zeros(C, H, W, C, H, W, dtype=torch.float32)
    i, j = torch.arange(H), torch.arange(W)
    for p in range(kh):
        ii = i + p - kh // 2                                          # output row i reads input row i + p - kh // 2
        vi = (ii >= 0) & (ii < H)
        for q in range(kw):
            jj = j + q - kw // 2
            vj = (jj >= 0) & (jj < W)
            oi, oj = torch.meshgrid(i[vi], j[vj], indexing="ij")
            si, sj = torch.meshgrid(ii[vi], jj[vj], indexing="ij")
            for c in range(C):
                a[c, oi, oj, c, si, sj] = kernel[p, q]
    return a.view(C * H * W, C * H * W)


def downsample(shape, factor):
    """The (C (H / factor) (W / factor), C H W) float32 matrix of mean pooling over factor x factor blocks: what
    ``torch.nn.functional.avg_pool2d(x, factor)`` does."""
    C, H, W = _chw(shape)
    f = int(factor)
    if f < 1 or H % f or W % f:
        raise ValueError(f"factor = {factor} must be a positive integer that divides H = {H} and W = {W}")
    a = torch.zeros(C, H // f, W // f, C, H // f, f, W // f, f, dtype=torch.float32)
    c, i, j = torch.meshgrid(torch.arange(C), torch.arange(H // f), torch.arange(W // f), indexing="ij")
    a[c, i, j, c, i, :, j, :] = 1.0 / (f * f)
    return a.view(C * (H // f) * (W // f), C * H * W)
