"""CPU restatement of CIM's multi-task loss on CMU-MOSEI (track_mm/cim.py:198-213) on top of tests/cim_oracle.cim_forward:
Lce = cross entropy of logits2 (apply_bin), Lmulti = BCE-with-logits of logits7 against the multi-hot emo_label (apply_multi),
Lall = the sum of the terms switched on.  Gradients follow from autograd (None = untouched)."""
import torch
import torch.nn.functional as F

from tests.cim_oracle import cim_forward


def cim_mosei_loss_and_grads(P, batch, masks=None, apply_multi=True, apply_bin=True):
    """-> (dict(Lall, Lce, Lmulti), logits2, logits7, {name: grad or None}, intermediates)"""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    logits2, logits7, inter = cim_forward(Q, batch, masks)
    lce = F.cross_entropy(logits2, batch["label"])
    lmulti = F.binary_cross_entropy_with_logits(logits7, batch["emo_label"].float()) if apply_multi else logits7.new_zeros(())
    lall = (lce if apply_bin else 0) + (lmulti if apply_multi else 0)
    lall.backward()
    losses = dict(Lall=lall.detach(), Lce=lce.detach(), Lmulti=lmulti.detach())
    return losses, logits2.detach(), logits7.detach(), {k: (v.grad if v.grad is None else v.grad.detach()) for k, v in Q.items()}, inter
