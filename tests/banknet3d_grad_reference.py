"""The differentiable float64 model of the Conv3d bank net, the yardstick of the native backward pass (fnx_banknet3d_train.hip): the one
statement of tests/banknet_grad_reference.py, which reads the dimension off its input (x (B,2,D,H,W), inp (B,6,D,H,W), the layout of
ext.banknet3d_tape_layout, the 3D gradient blob), under the names the 3D tests use.
"""
from banknet_grad_reference import (BANK_TENSORS, FACTOR, LAYERS, OWN_FLOOR, PARAM_NAMES, RELU_NAMES, TAPE_NAMES, as_params, check_grads,
                                    e32_per_tensor, fluidnet_e32, fluidnet_forward, fluidnet_gradients, forward, gradients,
                                    masks_from_tape, split_blob, tape_views, worst_rel)

__all__ = ["BANK_TENSORS", "FACTOR", "LAYERS", "OWN_FLOOR", "PARAM_NAMES", "RELU_NAMES", "TAPE_NAMES", "as_params", "check_grads",
           "e32_per_tensor", "fluidnet_e32", "fluidnet_forward", "fluidnet_gradients", "forward", "gradients", "masks_from_tape",
           "split_blob", "tape_views", "worst_rel"]
