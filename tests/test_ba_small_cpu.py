"""osfm_ba_options::small_form and osfm_ba_small_limits, as far as they can be checked without a device: the field took
the place of `reserved`, so the struct the callers of ABI version 102 were built against is unchanged."""
import ctypes as C

from orthosfm_amd import ba, capi

# osfm_ba_options before the field had a name: four doubles, two ints, six doubles, six ints -- `reserved` the last
PARENT_SIZE, PARENT_RESERVED_OFFSET = 112, 108


def test_struct_size_and_offset_are_the_parents():
    assert C.sizeof(capi.BaOptions) == PARENT_SIZE
    assert capi.BaOptions.small_form.offset == PARENT_RESERVED_OFFSET
    assert capi.BaOptions.small_form.size == 4
    assert not hasattr(capi.BaOptions, "reserved")
    assert capi.BaOptions._fields_[-1][0] == "small_form"


def test_default_leaves_the_general_form():
    o = capi.BaOptions()
    o.small_form = 77
    capi.check(capi.lib.osfm_ba_options_default(C.byref(o)))
    assert o.small_form == 0
    assert ba.default_options().small_form == 0
    assert ba.default_options(small_form=2).small_form == 2
    assert ba.default_options(2, device=0).small_form == 2


def test_small_limits():
    cams, chunk, auto = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    capi.check(capi.lib.osfm_ba_small_limits(C.byref(cams), C.byref(chunk), C.byref(auto)))
    assert cams.value == 8
    assert chunk.value > 0
    assert auto.value >= 0
    assert ba.small_limits() == (cams.value, chunk.value, auto.value)
    # any pointer may be null
    capi.check(capi.lib.osfm_ba_small_limits(None, C.byref(chunk), None))


def test_pipeline_knows_the_two_local_solvers():
    import inspect

    import pytest

    from orthosfm_amd import pipeline as P
    assert inspect.signature(P.reconstruct).parameters["local_solver"].default == "general"
    assert inspect.signature(P.run_pose_estimation).parameters["local_solver"].default == "general"
    with pytest.raises(ValueError):
        P.run_pose_estimation(None, None, 0, local_solver="tiny")
