"""Deterministic, closed-form parameter values for fixtures that do not store their parameters (tests/golden/g16_*.npz).

fill(module) overwrites every parameter of `module` -- in the order of its sorted state_dict keys -- with

    value[t][e] = centre_t + amplitude_t * u(t, e),      u(t, e) = ((h(t, e) >> 40) - 2^23) / 2^23   in [-1, 1)

where t is the tensor's index among the sorted keys, e the element's row-major index in the tensor's LOGICAL shape (so the
channel-last storage of a HexPlane plane does not matter), and h a 64-bit integer mix.  The hash is integer arithmetic modulo
2^64; its top 24 bits minus 2^23 convert to float32 exactly, 2^-23 and every amplitude are powers of two (chosen from the
tensor's shape with integer comparisons only), so `amplitude * u` is exact and the one rounding left -- adding the centre, an
IEEE float32 addition -- is the same on every platform.  ref_harness.py (on the reference's modules) and the tests (on this
package's) therefore start from the same bits without a stored state_dict.

Buffers that are part of the model's definition (the box `aabb`, the `*_poc` frequency tables) are left as they are.
"""
import numpy as np
import torch

_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xD1B54A32D192ED03)
_M3 = np.uint64(0xD6E8FEB86659FD93)
_S32 = np.uint64(32)
_S40 = np.uint64(40)


def unit(tensor_index, count):
    """float32 [count]: u(tensor_index, 0 .. count-1), each a multiple of 2^-23 in [-1, 1)."""
    with np.errstate(over="ignore"):
        h = np.arange(count, dtype=np.uint64) * _M1 + np.full(count, tensor_index + 1, np.uint64) * _M2
        for _ in range(2):
            h ^= h >> _S32
            h *= _M3
        h ^= h >> _S32
    k = (h >> _S40).astype(np.int64) - (1 << 23)
    return k.astype(np.float32) * np.float32(2.0 ** -23)


def _pow2_at_most(num, den):
    """Largest 2^-e (e >= 0) with (2^-e)^2 <= num / den, by integer comparison."""
    e = 0
    while num * 4 ** e < den:
        e += 1
    return 2.0 ** -e


def rule(key, shape):
    """(centre, amplitude) of a state_dict entry, or None for the entries fill() leaves alone.
    Planes: 0.75 +- 1, so that the product over a level's six planes is O(0.1) with a spread over the points larger than its mean:
    the features, not the biases, drive the network, and what a head computes varies from point to point.
    Linear weights: twice the largest power of two below Xavier's bound sqrt(6 / (fan_in + fan_out)); biases: +- 2^-3.
    The last layer of the five residual heads (`*_deform.3`) and of the static_mlp mask: weights a sixteenth of that; the heads'
    bias +- 2^-5.  The residual a head adds then varies over the points by 1e-2 to 4e-2 of the input it is added to and stays below
    0.35 in size, where the last bits in which two float32 BLAS libraries disagree (about 1e-7 of the sum of a dot product's terms)
    stay below the absolute tolerance the fixtures' outputs are compared at (1e-7).  The rotation head's bias is +- 2^-1 instead:
    under apply_rotation its output is normalised after the quaternion product, which hands the output the head's RELATIVE error,
    and the exactly representable bias has to carry most of the head's size for that to stay below 1e-7 of a unit quaternion."""
    if key.endswith("aabb") or key.endswith("_poc"):
        return None
    if ".grids." in key:
        return 0.75, 1.0
    if key.endswith(".weight") and len(shape) == 2:
        amp = 2.0 * _pow2_at_most(6, int(shape[0]) + int(shape[1]))
        return 0.0, amp / 16 if key.endswith(("_deform.3.weight", "static_mlp.3.weight")) else amp
    if key.endswith(".bias"):
        if key.endswith("_deform.3.bias"):
            return 0.0, 0.5 if "rotations_deform" in key else 0.03125
        return 0.0, 0.125
    raise KeyError("param_fill: no rule for %s %s" % (key, tuple(shape)))


def fill(module):
    """Overwrite the parameters of `module` in place; returns the list of keys written."""
    sd = module.state_dict()
    written = []
    with torch.no_grad():
        for t, key in enumerate(sorted(sd)):
            r = rule(key, sd[key].shape)
            if r is None:
                continue
            centre, amp = r
            v = np.float32(centre) + np.float32(amp) * unit(t, sd[key].numel())
            sd[key].copy_(torch.from_numpy(v).reshape(sd[key].shape))
            written.append(key)
    return written
