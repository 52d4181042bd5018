"""ROILoopPool — Python surface of projects/WSL/wsl/layers/roi_loop_pool.py:9-62 on top of
libjtsm_hip.so (jtsm_roi_loop_pool_{forward,backward}_f32).

forward(input (B,C,H,W), rois (R,5)) -> (3R, C, PH, PW): the box, frame and context blocks of
ContextLocNet, each in roi order.  The output follows the input's memory format (channels_last in,
channels_last out).  float16 tensors are widened to float32 here and the result rounded back; max
pooling only selects values, so that is exact.  The implementation is layers/roi_pool.py's, with three row blocks.
"""
from .roi_pool import MaxPoolModule, MaxPoolOp

_OP = MaxPoolOp("ROILoopPool", 3, "jtsm_roi_loop_pool_forward_f32", "jtsm_roi_loop_pool_backward_workspace_bytes",
                "jtsm_roi_loop_pool_backward_f32")
roi_loop_pool_forward, roi_loop_pool_backward, roi_loop_pool = _OP.forward, _OP.backward, _OP.apply


class ROILoopPool(MaxPoolModule):
    op = _OP
