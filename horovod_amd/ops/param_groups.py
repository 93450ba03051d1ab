"""Parameter groups for layer-wise adaptive optimizers.

LARS and LAMB exclude biases and normalisation parameters from weight decay,
and with it (FusedLARS, FusedLAMB: no decay, no adaptation) from the trust
ratio.  split_decay_groups builds the two groups every user of them writes by
hand:

    opt = FusedLARS(split_decay_groups(model, 5e-5), lr=...)
"""
import torch


def split_decay_groups(module_or_named_params, weight_decay):
    """-> [{"params": [...], "weight_decay": weight_decay},
           {"params": [...], "weight_decay": 0.0}]

    Takes a torch.nn.Module or an iterable of (name, parameter) pairs.
    Parameters with ndim <= 1 (biases, BatchNorm/LayerNorm weights) go to the
    second group, the rest to the first; each keeps the order it came in.
    A parameter met twice (shared weights) is taken once.
    """
    if isinstance(module_or_named_params, torch.nn.Module):
        named = module_or_named_params.named_parameters()
    else:
        named = module_or_named_params
    decay, no_decay, seen = [], [], set()
    for _, p in named:
        if id(p) in seen:
            continue
        seen.add(id(p))
        (no_decay if p.ndim <= 1 else decay).append(p)
    return [{"params": decay, "weight_decay": weight_decay},
            {"params": no_decay, "weight_decay": 0.0}]
