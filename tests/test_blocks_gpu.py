"""The kernels' building blocks on the device (pbrt_hip_blocks_eval_device: a tiny kernel that calls cephes_poly.hpp, envmap_core.hpp and
kernel_math.hpp themselves) over the input sets of tests/blocks_ref.py: every output equal to the oracle's bit for bit -- NaN and inf
included --, and the float64 bounds of tests/test_blocks_host.py on the device's own values."""
import numpy as np
import pytest

import blocks_ref as br
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24  # elements per call of the hook


def _device(gpu, op, x):
    from pbrt_amd import api
    return np.concatenate([api.blocks_eval(op, x[a:a + CHUNK]) for a in range(0, len(x), CHUNK)])


@pytest.mark.parametrize("op", br.ALL_OPS)
def test_device_blocks_equal_the_oracle_and_meet_the_float64_bounds(gpu, oracle, op):
    """one evaluation per op (the strided sets of the polynomials hold 2^25 patterns: two calls of 2^24), then the comparison with the
    oracle and the checks against float64 -- the same functions and bounds the CPU tests run on the oracle"""
    x, aux = br.inputs(op)
    got = _device(gpu, op, x)
    assert_bit_equal(got, oracle.blocks_eval(op, x), op)
    wild = br.wild_inputs(op)
    if wild is not None:
        assert_bit_equal(_device(gpu, op, wild), oracle.blocks_eval(op, wild), op + " off its domain")
    print(op, len(x), "inputs:", br.check(op, x, aux, got))


def test_fresnel_clamps_a_cosine_above_one(gpu, oracle):
    x = br.fresnel_above_one_inputs()
    got = _device(gpu, "FRESNEL", x)
    assert_bit_equal(got, oracle.blocks_eval("FRESNEL", x), "FRESNEL above 1")
    br.check_fresnel_above_one(x, got)


def test_device_hook_refuses_an_unknown_op(gpu):
    from pbrt_amd import _lib
    a = np.zeros(4, np.float32)
    with pytest.raises(_lib.PbrtHipError) as e:
        _lib.check(_lib.lib().pbrt_hip_blocks_eval_device(0, 99, 4, a.ctypes.data_as(_lib._pf), a.ctypes.data_as(_lib._pf)), "pbrt_hip_blocks_eval_device")
    assert e.value.code == -1
