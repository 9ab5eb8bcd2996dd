"""Float64 oracle of the evaluation metrics.  TEST INFRASTRUCTURE ONLY.

SSIM is ``oracle.train_oracle.ssim`` (the restatement of pytorch_msssim's published algorithm that the training loss is
tested against) run in double; MSE, L1 and PSNR are numpy on the same float32 inputs taken to double: PSNR =
-10 log10(mse), torchmetrics' PeakSignalNoiseRatio(data_range=1.0), +inf where mse == 0."""
import numpy as np
import torch

from oracle import train_oracle as TO


def metrics(image: torch.Tensor, target: torch.Tensor) -> np.ndarray:
    """image: float32 [H, W, 3 or 4] (a fourth channel is ignored); target: float32 [H, W, 3] -> float64
    {mse, l1, ssim, psnr}."""
    assert image.dtype == torch.float32 and target.dtype == torch.float32
    x, y = image[:, :, :3].double(), target.double()
    d = (x - y).numpy()
    mse, l1 = float(np.mean(d * d)), float(np.mean(np.abs(d)))
    with np.errstate(divide="ignore"):
        psnr = float(-10.0 * np.log10(mse))
    return np.array([mse, l1, float(TO.ssim(x, y)), psnr], dtype=np.float64)
