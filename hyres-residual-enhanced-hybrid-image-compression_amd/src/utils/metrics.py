"""Evaluation metrics (src/utils/metrics.py:6-53) — the reference's ``CompressionMetrics`` with its method names and
return types. MS-SSIM runs on the HIP kernels of hyres_hip.metrics (pytorch_msssim's ms_ssim at its defaults; CPU
tensors take the host twin of the same arithmetic). Neither ``pytorch_msssim`` nor ``lpips`` is imported.

Two deliberate differences from the reference:
  * ``psnr`` is 10*log10(1/mse) per image, averaged — the reference's ``-10*log10(mse)`` is the same number; the
    CLI's wrong ``-10*log10(mse*255^2)`` (src/inference.py:123-125) is not repeated here;
  * ``lpips`` raises: LPIPS needs the AlexNet weights and the learned linear heads of the ``lpips`` package, which
    are not available offline, and a stand-in with other weights would report a different metric under the same name.
    ``compute_all`` therefore returns psnr and ms-ssim only."""
import torch

from hyres_hip.metrics import ms_ssim

__all__ = ["CompressionMetrics"]


class CompressionMetrics:
    """Common metrics for image compression evaluation."""

    def __init__(self, device='cuda'):
        self.device = device

    def psnr(self, x, y):
        """Peak Signal-to-Noise Ratio of [B,3,H,W] tensors in [0,1]: mean over the batch of 10*log10(1/mse)."""
        mse = torch.mean((x - y) ** 2, dim=[1, 2, 3])
        return (10 * torch.log10(1.0 / mse)).mean().item()

    def msssim(self, x, y):
        """MS-SSIM (data_range 1.0, five levels) of [B,3,H,W] tensors in [0,1], min(H, W) > 160."""
        return ms_ssim(x, y, data_range=1.0).item()

    def lpips(self, x, y):
        raise RuntimeError("CompressionMetrics.lpips: the LPIPS (AlexNet) weights are not available offline; "
                           "this port ships no substitute for them")

    def compute_all(self, x, y):
        """psnr and ms-ssim; 'lpips' is left out because its weights are not available offline (see ``lpips``)."""
        return {
            'psnr': self.psnr(x, y),
            'ms-ssim': self.msssim(x, y),
        }
