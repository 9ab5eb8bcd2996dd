"""float64 restatement of the opacity-entropy regulariser (scripts/train.py:71-75) for tinysplat_amd.surface:
the expression evaluated in float64 from the float32 logits (or in float32, as the script runs it), its gradient by
autograd."""
import torch


def opacity_entropy_oracle(opacities, dtype=torch.float64, weight=1.0):
    """-> (L_o, d(weight * L_o)/d opacities) in ``dtype`` (float32: the reference's own evaluation, op for op, with
    ``weight`` = lambda_opacity)."""
    x = torch.as_tensor(opacities).to(dtype).requires_grad_(True)
    o = torch.sigmoid(x)
    loss = -(o * torch.log(o + 1e-10) + (1 - o) * torch.log(1 - o + 1e-10)).mean()
    (weight * loss).backward()
    return loss.detach(), x.grad
