"""CPU: the argument checks of dbhip_inlist_create (include/dbhip.h a23) need no device — every refusal is decided on the host before
the set is copied anywhere — so they are tested here through the raw binding, without dbhip_init: the limits, the types, the offsets.
tests/test_gpu_inlist.py repeats them on the device beside the sets that are accepted."""
import ctypes as C

from databend_amd import _lib as T


def create(dtype, values, offsets, n, has_out=True):
    h = C.c_void_p()
    rc = T.lib().dbhip_inlist_create(C.c_int32(dtype), C.c_uint8(0), C.c_uint8(0), values, offsets, C.c_int32(n), C.c_int32(0), C.byref(h) if has_out else None)
    return rc, h


def test_refusals_need_no_device():
    vals = (C.c_int64 * 2000)(*range(2000))
    for dtype, values, offsets, n, has_out, code, what in [
        (T.T_BOOL, vals, None, 2, True, T.ERR_UNSUPPORTED, "Boolean"),
        (T.T_DEC256, vals, None, 2, True, T.ERR_UNSUPPORTED, "Decimal256"),
        (T.T_I64, vals, None, T.IN_MAX_ITEMS + 1, True, T.ERR_UNSUPPORTED, "more than 1024 elements"),
        (T.T_I64, None, None, 2, True, T.ERR_INVALID, "NULL values"),
        (T.T_I64, vals, None, -1, True, T.ERR_INVALID, "a negative count"),
        (0, vals, None, 2, True, T.ERR_INVALID, "type 0"),
        (99, vals, None, 2, True, T.ERR_INVALID, "type 99"),
        (T.T_I64, vals, None, 2, False, T.ERR_INVALID, "NULL out"),
        (T.T_STRING, vals, None, 2, True, T.ERR_INVALID, "a String list without offsets"),
        (T.T_STRING, vals, (C.c_uint32 * 3)(0, 5, 4), 2, True, T.ERR_INVALID, "descending offsets"),
        (T.T_STRING, vals, (C.c_uint32 * 2)(0, T.IN_MAX_ITEM_BYTES + 1), 1, True, T.ERR_UNSUPPORTED, "an element of 256 bytes"),
        (T.T_STRING, (C.c_uint8 * 16500)(), (C.c_uint32 * 67)(*[250 * j for j in range(67)]), 66, True, T.ERR_UNSUPPORTED, "16,500 bytes of long elements"),
    ]:
        rc, h = create(dtype, values, offsets, n, has_out)
        assert rc == code, (what, rc)
        assert h.value is None, what
        msg = T.lib().dbhip_last_error()
        assert msg and b"DBHIP_IN" not in msg, (what, msg)


def test_an_empty_list_is_a_set_without_a_device_image():
    """IN () has nothing to copy: create succeeds before any device call, on the COMPARE path (BITS for the narrow types has a bitmap)"""
    for dtype in (T.T_I32, T.T_I64, T.T_F64, T.T_DEC128, T.T_STRING):
        rc, h = create(dtype, None, None, 0)
        assert rc == T.OK and h.value, dtype
        assert T.lib().dbhip_inlist_path(h) == T.IN_PATH_COMPARE
        assert T.lib().dbhip_inlist_destroy(h) == T.OK
    assert T.lib().dbhip_inlist_path(None) == -T.ERR_INVALID and T.lib().dbhip_inlist_destroy(None) == T.OK
