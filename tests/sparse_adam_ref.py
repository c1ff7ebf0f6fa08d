"""Torch restatement of the row-sparse Adam step (splatco_amd.adam.FusedAdam.step(visible=...), csrc/adam.hip
adam_rows_kernel): torch's single-tensor Adam formulas (torch/optim/adam.py _single_tensor_adam, the ones csrc/adam.hip's
header quotes) applied to the GATHERED visible rows of parameter, gradient and moments, the results scattered back; rows
outside the mask are never read or written.  `step` is the tensor's counter and advances every step, whichever rows were
visible, so the bias corrections are the tensor's.  fp32, any device, no product code."""
import torch


def adam_rows_torch(p, g, m, v, step, lr, beta1, beta2, eps, rows=None):
    """One step on rows `rows` (a LongTensor of row indices; None: every element) of p / m / v, in place.  step: the
    tensor's step count INCLUDING this step."""
    with torch.no_grad():
        if rows is None:
            P, G, M, V = p, g, m, v
        else:
            P, G, M, V = p[rows], g[rows], m[rows], v[rows]
        M.lerp_(G, 1 - beta1)
        V.mul_(beta2).addcmul_(G, G, value=1 - beta2)
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        step_size = lr / bias_correction1
        bias_correction2_sqrt = bias_correction2 ** 0.5
        denom = (V.sqrt() / bias_correction2_sqrt).add_(eps)
        P.addcdiv_(M, denom, value=-step_size)
        if rows is not None:
            p[rows], m[rows], v[rows] = P, M, V


class SparseAdamRef:
    """groups: [{"params": [...], "lr": ..., "row_sparse": bool (optional)}]; state[p] = {"step", "exp_avg", "exp_avg_sq"}.
    step(visible): row-sparse groups are stepped on the rows `visible` marks (nonzero), all other groups on every element;
    visible=None: every group densely.  A parameter without a gradient is skipped and its step count does not move."""

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8):
        self.param_groups = [dict(g) for g in groups]
        self.betas, self.eps = betas, eps
        self.state = {}

    def step(self, visible=None):
        rows = None if visible is None else torch.nonzero(visible != 0).reshape(-1)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state.setdefault(p, {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)})
                st["step"] += 1
                adam_rows_torch(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"], float(group["lr"]), self.betas[0],
                                self.betas[1], self.eps, rows if group.get("row_sparse", False) else None)
