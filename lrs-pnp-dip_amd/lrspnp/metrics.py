"""Quality metrics of the reference (not timed), on the device: per-band PSNR with its
10*log10(255/RMSE) definition and the band mean (main_LRS_PnP.py:40-58, :379-384) on the HIP kernel
lrs_psnr_bands_f32, and MSSIM (pytorch_ssim.ssim, main_LRS_PnP_DIP_1-LiP.py:480-481) on lrs_ssim_f32.
Nothing leaves the GPU but the final scalar."""
from __future__ import annotations

import torch


def fold(X: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """X (H*W, B), row p = i + H*j  ->  (B, H, W)."""
    B = X.shape[1]
    return X.reshape(W, H, B).permute(2, 1, 0)


def psnr_bands(X: torch.Tensor, clean_bhw: torch.Tensor) -> torch.Tensor:
    """Per-band PSNR (device float64 [B]) of the unfolded X (P x B) against clean (B, H, W)."""
    from . import ops
    from ._lib import check, device_lib, ptr, sptr
    B, H, W = clean_bhw.shape
    C = ops.image_to_unfolded(clean_bhw.contiguous().float(), H, W)
    Xc = X.contiguous().float()
    L = device_lib()
    P = H * W
    ws = torch.empty(int(L.lrs_psnr_workspace(P, B)), dtype=torch.uint8, device=X.device)
    out = torch.empty(B, dtype=torch.float64, device=X.device)
    check(L.lrs_psnr_bands_f32(ptr(Xc), ptr(C), P, B, ptr(out), ptr(ws), ws.numel(), sptr()), "lrs_psnr_bands_f32")
    return out


def mpsnr(X: torch.Tensor, clean_bhw: torch.Tensor) -> float:
    return float(psnr_bands(X, clean_bhw).mean())


def quality(X: torch.Tensor, clean_bhw: torch.Tensor, region: torch.Tensor | None = None) -> dict:
    """MPSNR, SAM (degrees), relative error and the per-band PSNR of the unfolded X (P x B) against clean
    (B, H, W), over every entry or over region (P x B, nonzero = counted; 1 - M scores the hole alone): one
    fused pass (ops.cube_quality, which states the definitions) and one read of the device at the end.
    LrsPnP.run() is the form that scores every iteration without a host sync."""
    from . import ops
    B, H, W = clean_bhw.shape
    C = ops.image_to_unfolded(clean_bhw.contiguous().float(), H, W)
    if region is not None:
        region = (region != 0).to(torch.uint8).contiguous()
    out = torch.empty(4 + B, dtype=torch.float64, device=X.device)
    ops.cube_quality(X.contiguous().float(), C, region, q=out[:4], psnr_bands=out[4:])
    h = out.cpu().numpy()
    return dict(mpsnr=float(h[0]), sam_deg=float(h[1]), rel_err=float(h[2]), psnr_bands=h[4:].copy())


def mssim(img1: torch.Tensor, img2: torch.Tensor) -> float:
    """pytorch_ssim.ssim(img1, img2) for (B, H, W) (or (1, B, H, W)) float32 device images."""
    from ._lib import check, device_lib, ptr, sptr
    a = img1.reshape(-1, *img1.shape[-2:]).contiguous().float()
    b = img2.reshape(-1, *img2.shape[-2:]).contiguous().float()
    C, H, W = a.shape
    acc = torch.zeros(1, dtype=torch.float64, device=a.device)
    check(device_lib().lrs_ssim_f32(ptr(a), ptr(b), C, H, W, ptr(acc), sptr()), "lrs_ssim_f32")
    return float(acc) / (C * H * W)
