"""The optimizer of the reference's training loop on the HIP path.

The reference builds `torch.optim.Adam` over two parameter groups, the depth network's and the pose network's, each with its own
weight decay, and halves `lr` through `param_groups` along its schedule (src/kbnet.py:360-369, 439-453).  `Adam` below is that
optimizer with the update itself in one multi-tensor HIP kernel (ops.adam_step, csrc/adam.hip): one call for every parameter of
every group instead of a dozen torch._foreach_* launches, each a pass over all the weights.

    optimizer = kb.optim.Adam([{'params': depth_model.parameters(), 'weight_decay': w_weight_decay_depth},
                               {'params': pose_model.parameters(), 'weight_decay': w_weight_decay_pose}], lr=learning_rate)
    ...
    optimizer.zero_grad(); loss.backward(); optimizer.step()
"""

from __future__ import annotations

import torch

from . import ops

__all__ = ["Adam"]

# torch.optim.Adam options this optimizer does not implement, with the only value each may have (None: left to the optimizer)
_REFUSED = {"amsgrad": (False,), "maximize": (False,), "foreach": (None, False), "capturable": (False,), "differentiable": (False,),
            "fused": (None, False), "decoupled_weight_decay": (False,)}


def _check_group(group: dict) -> None:
    for name, allowed in _REFUSED.items():
        value = group.get(name, allowed[0])
        if not any(value is a for a in allowed):
            raise ValueError(f"kbnet_amd.optim.Adam does not support {name}={value!r}: the HIP step is torch's single-tensor Adam with "
                             "L2 weight decay (csrc/adam.hip)")
    if isinstance(group["lr"], torch.Tensor):
        raise ValueError("kbnet_amd.optim.Adam does not support a tensor lr: the bias corrections are host numbers (set lr as a float "
                         "through param_groups)")
    if not 0.0 <= group["lr"]:
        raise ValueError(f"Invalid learning rate: {group['lr']}")
    if not 0.0 <= group["eps"]:
        raise ValueError(f"Invalid epsilon value: {group['eps']}")
    beta1, beta2 = group["betas"]
    if isinstance(beta1, torch.Tensor) or isinstance(beta2, torch.Tensor):
        raise ValueError("kbnet_amd.optim.Adam does not support tensor betas")
    if not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
        raise ValueError(f"Invalid betas: {group['betas']}")
    if not 0.0 <= group["weight_decay"]:
        raise ValueError(f"Invalid weight_decay value: {group['weight_decay']}")


def load_checkpoint_state(optimizer, checkpoint: dict) -> None:
    """The optimizer half of the models' restore_model(path, optimizer): the checkpoint's `optimizer_state_dict` into `optimizer`
    when there is an optimizer and the dict is not empty (save_model(..., optimizer=None) writes an empty one).  Errors of
    load_state_dict propagate."""
    state = checkpoint.get("optimizer_state_dict")
    if optimizer is not None and state:
        optimizer.load_state_dict(state)


class Adam(torch.optim.Optimizer):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay)` with the step on the HIP kernel of ops.adam_step: Adam with L2
    weight decay, as the reference trains (src/kbnet.py:360-369).  Param groups with their own lr / betas / eps / weight_decay, and
    `lr` changed through `param_groups` between steps, work as in torch.

    The state is interchangeable with torch's: per parameter `step` (an fp32 CPU scalar tensor), `exp_avg` and `exp_avg_sq`
    (preserve_format zeros like the parameter); `defaults` and `param_groups` carry torch.optim.Adam's keys in its order, so
    `state_dict()` of either optimizer loads into the other, and the `optimizer_state_dict` of a reference checkpoint loads
    (KBNetModel.restore_model(path, optimizer)).

    A parameter whose `.grad` is None is skipped: no state is made for it and its `step` does not advance (KBNet's
    calibrated_backprojection4.conv_image is never used by the forward).  `step()` hands every other parameter of every group to
    ONE ops.adam_step call, which also bumps the parameters' version counters (see its docstring: the packed-weight caches
    follow them).

    Refused with a ValueError that names the option, at construction and -- for values that arrive through load_state_dict -- in
    step(): amsgrad, maximize, capturable, differentiable, decoupled_weight_decay, foreach=True, fused=True, a tensor lr, a closure.
    Parameters must be dense fp32 HIP tensors; CPU parameters raise KbnError in step().  step() cannot be captured into a HIP
    graph: the bias corrections 1 - beta^t are host numbers computed per call."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        _check_group(defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:
            _check_group(group)

    def __setstate__(self, state):
        """As torch.optim.Adam.__setstate__: a state dict written by an older torch lacks the newer group keys and may hold `step`
        as a Python number.  `step` is kept where torch keeps it without capturable / fused: an fp32 scalar on the CPU."""
        super().__setstate__(state)
        for group in self.param_groups:
            for name, allowed in _REFUSED.items():
                group.setdefault(name, allowed[0])
            for p in group["params"]:
                s = self.state.get(p, {})
                if len(s) != 0 and (not torch.is_tensor(s["step"]) or s["step"].is_cuda):
                    # (a checkpoint read with map_location=<device>, as restore_model reads it, brings `step` to the device)
                    s["step"] = torch.tensor(float(s["step"]), dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("kbnet_amd.optim.Adam does not support a closure: call loss.backward() before step()")
        params, grads, exp_avgs, exp_avg_sqs, steps, lrs, betas, epss, wds, counts = [], [], [], [], [], [], [], [], [], []
        for group in self.param_groups:
            _check_group(group)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if "max_exp_avg_sq" in state:
                    raise ValueError("kbnet_amd.optim.Adam does not support amsgrad=True (the loaded state holds max_exp_avg_sq)")
                step = state["step"]
                if step.is_cuda:
                    raise ValueError("kbnet_amd.optim.Adam does not support capturable=True (the loaded state holds `step` on the device)")
                params.append(p)
                grads.append(p.grad)
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                counts.append(step)
                steps.append(step.item() + 1.0)
                lrs.append(group["lr"])
                betas.append(group["betas"])
                epss.append(group["eps"])
                wds.append(group["weight_decay"])
        if not params:
            return None
        ops.adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr=lrs, betas=betas, eps=epss, weight_decay=wds)
        torch._foreach_add_(counts, 1)    # the CPU step counts, after the launch: a refused tensor leaves every count where it was
        return None
