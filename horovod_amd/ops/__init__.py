from horovod_amd.ops.fused_sgd import FusedSGD  # noqa: F401
from horovod_amd.ops.fused_adamw import FusedAdamW  # noqa: F401
from horovod_amd.ops.fused_lamb import FusedLAMB  # noqa: F401
from horovod_amd.ops.fused_lars import FusedLARS  # noqa: F401
from horovod_amd.ops.param_groups import split_decay_groups  # noqa: F401
from horovod_amd.ops.fused_bn import (FusedBNAddReLU,  # noqa: F401
                                      FusedBNReLU)
from horovod_amd.ops.fused_ln import (FusedDropoutAddLayerNorm,  # noqa: F401
                                      FusedLayerNorm,
                                      dropout_add_layer_norm)
from horovod_amd.ops.clip import clip_grad_norm_  # noqa: F401
