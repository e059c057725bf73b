"""The test seam of the field arithmetic (lw_hip_field_pointwise_device, include/lw_hip.h): one primitive of
csrc/field.cuh per row of device-resident torch tensors, the returned limbs written to t_out as they are."""
from . import _lib as L
from .errors import check


def field_pointwise_device(field, op, t_a, t_b, n, t_out, stream=None):
    """field: L.PW_FIELD_*; op: L.FIELD_OP_*; t_b: None for the ops with one operand.  Rows and operand domains: see the
    header.  For FIELD_OP_MUL_LAZY_UNIFORM t_a holds the one row every work-item reads."""
    check(L.lib().lw_hip_field_pointwise_device(field, op, L.device_ptr(t_a), L.device_ptr(t_b) if t_b is not None else None, n,
                                                L.device_ptr(t_out), L.stream_ptr(stream)))
    return t_out
