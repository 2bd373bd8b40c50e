"""The kernels' building blocks on the device (pbrt_hip_blocks_eval_device: a tiny kernel that calls cephes_poly.hpp, envmap_core.hpp,
kernel_math.hpp, kernel_path.hpp's sample_light and the walk's node step and triangle test -- kernel_walk.hpp quad_step, quad_nearest.inc, tri_test.inc -- themselves) over the input sets of tests/blocks_ref.py: every output equal to the oracle's bit for bit -- NaN and inf
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


def test_the_two_fma_forms_of_the_node_step_agree(gpu):
    """QUAD_STEP (scalar fmas, the kernels without an overflow stack) and QUAD_STEP_PK (packed) give the same bits, NaN and inf included"""
    x, _ = br.inputs("QUAD_STEP")
    assert_bit_equal(_device(gpu, "QUAD_STEP", x), _device(gpu, "QUAD_STEP_PK", x), "QUAD_STEP against QUAD_STEP_PK")


@pytest.mark.parametrize("size", br.wr.TRI_SIZES)
def test_triangle_ladder_on_the_device(gpu, oracle, size):
    """the 27 rungs of one size (tests/test_blocks_host.py test_triangle_test_against_float64): bit-equal to the oracle, the same bounds"""
    x, parts = br.wr.tri_hit_inputs(size)
    got = _device(gpu, "TRI_HIT", x)
    assert_bit_equal(got, oracle.blocks_eval("TRI_HIT", x), f"TRI_HIT size {size}")
    table = br.wr.check_tri_hit(parts, x, got)
    print(size, {rung: (m["robust"], m["ratio_t"], m["ratio_u"], m["ratio_v"]) for rung, m in table.items() if m["asserted"]})


def test_fresnel_clamps_a_cosine_above_one(gpu, oracle):
    x = br.fresnel_above_one_inputs()
    got = _device(gpu, "FRESNEL", x)
    assert_bit_equal(got, oracle.blocks_eval("FRESNEL", x), "FRESNEL above 1")
    br.check_fresnel_above_one(x, got)


def test_device_hook_refuses_an_unknown_op(gpu):
    from pbrt_amd import _lib
    from pbrt_amd import api
    a = np.zeros(64, np.float32)
    for op in (len(api.BLOCK_OPS), 99):  # PBRT_HIP_BLOCK_COUNT itself, and beyond
        with pytest.raises(_lib.PbrtHipError) as e:
            _lib.check(_lib.lib().pbrt_hip_blocks_eval_device(0, op, 1, a.ctypes.data_as(_lib._pf), a.ctypes.data_as(_lib._pf)), "pbrt_hip_blocks_eval_device")
        assert e.value.code == -1
    assert len(api.BLOCK_OPS) == 15
