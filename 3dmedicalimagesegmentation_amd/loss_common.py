"""What the loss modules share (seg_losses.SegLoss, topk_loss.TopKLoss / DiceTopKLoss, distance.BoundaryLoss / HausdorffDTLoss):
the argument checks of their constructors, the checks of a call's shapes, the class weights as a device buffer, and the one-element
device scalar a captured step reads.  The forward prologue of their autograd Functions is functional._loss_inputs."""
import torch


def require_mean(reduction):
    if reduction != "mean":
        raise NotImplementedError(f"reduction={reduction!r}: the HIP loss family implements reduction='mean'")


def activation_form(to_onehot_y, softmax, sigmoid, required=True):
    """-> multilabel.  The two input forms of the family: (to_onehot_y, softmax) on class ids and (not to_onehot_y, sigmoid) on a
    float mask; required=False: a loss that reads the raw logits only takes either target form without an activation."""
    if softmax and sigmoid:
        raise ValueError("softmax=True and sigmoid=True exclude each other")
    if required and (bool(to_onehot_y), bool(softmax), bool(sigmoid)) not in ((True, True, False), (False, False, True)):
        raise NotImplementedError("the HIP loss family implements to_onehot_y=True with softmax=True and to_onehot_y=False with "
                                  f"sigmoid=True; got to_onehot_y={to_onehot_y}, softmax={softmax}, sigmoid={sigmoid}")
    return not to_onehot_y


def class_weight_list(class_weight):
    class_weight = [float(w) for w in (class_weight.tolist() if isinstance(class_weight, torch.Tensor) else class_weight)]
    if not class_weight or min(class_weight) < 0:
        raise ValueError("class_weight must hold one non-negative entry per channel")
    return class_weight


def weights_on(cache, class_weight, device):
    """class_weight (a list, or None) as a float32 buffer on `device`, created at first use and kept in `cache` (device -> tensor)"""
    if class_weight is None or device.type != "cuda":
        return None
    w = cache.get(device)
    if w is None:
        w = cache[device] = torch.tensor(class_weight, dtype=torch.float32, device=device)
    return w


def check_call(input, target, cfg, class_weight=None):
    """the shapes of one call against a module's cfg (multilabel; include_background where the loss has it) and class weights"""
    if cfg["multilabel"]:
        if target.shape != input.shape:
            raise ValueError("to_onehot_y=False needs a target shaped like the logits [B,C,*spatial]")
    elif target.shape[1] != 1:
        raise ValueError("target must be [B,1,*spatial] class indices (to_onehot_y=True)")
    if not cfg.get("include_background", 1) and input.shape[1] == 1:
        raise ValueError("include_background=False needs more than one channel")
    if class_weight is not None and len(class_weight) != input.shape[1]:
        raise ValueError(f"class_weight has {len(class_weight)} entries for {input.shape[1]} channels")


def device_scalar(value):
    """one float32 in device memory (on the current device; the CPU where there is none), to be registered as a buffer"""
    return torch.full((1,), float(value), dtype=torch.float32, device="cuda" if torch.cuda.is_available() else "cpu")


def scalar_on(module, name, input, what):
    """module.<name> (a device_scalar buffer) on the device of `input`: moved there at first use, never while a stream captures"""
    t = getattr(module, name)
    if t.device != input.device and input.is_cuda:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} is not on the logits' device yet: run the loss once before capturing it")
        t = t.to(input.device)
        setattr(module, name, t)
    return t
