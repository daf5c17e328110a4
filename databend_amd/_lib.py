"""ctypes binding of include/dbhip.h (the drop-in C-ABI).  Fails loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class DbhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dbhip error {code}: {msg}")
        self.code = code


# status codes (include/dbhip.h)
OK, ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_ROW_ERRORS, ERR_OVERFLOW, ERR_CAPACITY, ERR_UNSUPPORTED, ERR_CANCELLED = range(9)

# dbhip_type
T_BOOL, T_I8, T_I16, T_I32, T_I64, T_U8, T_U16, T_U32, T_U64, T_F32, T_F64, T_DATE, T_TIMESTAMP, T_DEC64, T_DEC128, T_STRING, T_DEC256 = range(1, 18)
OP_PLUS, OP_MINUS, OP_MULTIPLY, OP_DIVIDE, OP_INTDIV, OP_MODULO, OP_DIV0, OP_DIVNULL = range(8)
CMP_EQ, CMP_NOTEQ, CMP_LT, CMP_LTE, CMP_GT, CMP_GTE = range(6)
AGG_COUNT, AGG_SUM, AGG_MIN, AGG_MAX = range(4)
VEC_COSINE, VEC_L2, VEC_DOT, VEC_L1, VEC_NORM = range(5)


class Col(C.Structure):
    """dbhip_col"""
    _fields_ = [
        ("type", C.c_int32), ("is_scalar", C.c_int32), ("data", C.c_void_p),
        ("validity", C.c_void_p), ("validity_offset", C.c_int64),
        ("buffers", C.c_void_p), ("n_buffers", C.c_int32),
        ("precision", C.c_uint8), ("scale", C.c_uint8), ("_pad", C.c_uint8 * 2),
    ]


EX_LOAD, EX_CONST, EX_PLUS, EX_MINUS, EX_MULTIPLY, EX_DIVIDE, EX_EQ, EX_NOTEQ, EX_LT, EX_LTE, EX_GT, EX_GTE, EX_AND, EX_OR, EX_NOT, EX_CAST, EX_IF, EX_IS_TRUE, EX_DT_PART, EX_DT_TRUNC = range(20)


class ExprIns(C.Structure):
    """dbhip_expr_ins"""
    _fields_ = [("op", C.c_int32), ("dst", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("type", C.c_int32),
                ("precision", C.c_uint8), ("scale", C.c_uint8), ("_pad", C.c_uint8 * 2), ("imm", C.c_uint64)]


class AggProgram(C.Structure):
    """dbhip_agg_program"""
    _fields_ = [("prog", C.c_void_p), ("n_ins", C.c_int32), ("inputs", C.c_void_p), ("n_inputs", C.c_int32), ("filter_reg", C.c_int32),
                ("arg_regs", C.c_void_p)]


class PqInfo(C.Structure):
    """dbhip_pq_info"""
    _fields_ = [("num_values", C.c_int64), ("num_nulls", C.c_int64), ("out_type", C.c_int32), ("has_validity", C.c_int32),
                ("out_bytes", C.c_int64), ("validity_bytes", C.c_int64), ("n_pages", C.c_int64), ("n_dict_values", C.c_int64),
                ("image_bytes", C.c_int64)]


class PqNode(C.Structure):
    """dbhip_pq_node"""
    _fields_ = [("kind", C.c_int32), ("nullable", C.c_int32)]


class PqNodeOut(C.Structure):
    """dbhip_pq_node_out"""
    _fields_ = [("offsets_dev", C.c_void_p), ("validity_dev", C.c_void_p), ("items", C.c_int64), ("nulls", C.c_int64)]


# dbhip_pq_node.kind
PQ_LIST, PQ_STRUCT = 1, 2

# parquet.thrift Type numbers
PQ_BOOLEAN, PQ_INT32, PQ_INT64, PQ_INT96, PQ_FLOAT, PQ_DOUBLE, PQ_BYTE_ARRAY, PQ_FLBA = range(8)
# parquet.thrift CompressionCodec numbers the library decodes
PQ_UNCOMPRESSED, PQ_SNAPPY, PQ_ZSTD, PQ_LZ4_RAW = 0, 1, 6, 7


class AggDesc(C.Structure):
    """dbhip_agg_desc"""
    _fields_ = [("kind", C.c_int32), ("arg_type", C.c_int32), ("arg_precision", C.c_uint8),
                ("arg_scale", C.c_uint8), ("arg_nullable", C.c_uint8), ("_pad", C.c_uint8)]


class WindowRows(C.Structure):
    """dbhip_window_rows"""
    _fields_ = [("n", C.c_int64), ("part_start", C.c_void_p), ("part_end", C.c_void_p), ("peer_start", C.c_void_p), ("peer_end", C.c_void_p)]


class WindowFrame(C.Structure):
    """dbhip_window_frame"""
    _fields_ = [("units", C.c_int32), ("start_kind", C.c_int32), ("end_kind", C.c_int32), ("_pad", C.c_int32),
                ("start_offset", C.c_int64), ("end_offset", C.c_int64)]


WIN_ROWS, WIN_RANGE = 0, 1
WIN_UNBOUNDED_PRECEDING, WIN_PRECEDING, WIN_CURRENT_ROW, WIN_FOLLOWING, WIN_UNBOUNDED_FOLLOWING = range(5)
WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_PERCENT_RANK, WIN_CUME_DIST, WIN_NTILE = range(6)
WIN_FIRST_VALUE, WIN_LAST_VALUE, WIN_NTH_VALUE = range(3)

# dbhip_like_kind_t, the flags of dbhip_like / dbhip_str_match, and DBHIP_LIKE_LONG_BYTES
LIKE_EQUALS, LIKE_PREFIX, LIKE_SUFFIX, LIKE_CONTAINS, LIKE_SEGMENTS = range(5)
LIKE_NEGATE, LIKE_UNIT_BYTE = 1, 2
LIKE_LONG_BYTES = 256


class Tz(C.Structure):
    """dbhip_tz"""
    _fields_ = [("offset_s", C.c_int32), ("n_transitions", C.c_int32), ("at_utc_s", C.c_void_p), ("offset_after_s", C.c_void_p)]


# dbhip_dt_part_t, dbhip_dt_unit_t and the flag of dbhip_dt_trunc
(DT_PART_YEAR, DT_PART_QUARTER, DT_PART_MONTH, DT_PART_DAY, DT_PART_DAY_OF_YEAR, DT_PART_DOW_ISO, DT_PART_DOW_SUNDAY0, DT_PART_ISO_YEAR,
 DT_PART_ISO_WEEK, DT_PART_HOUR, DT_PART_MINUTE, DT_PART_SECOND, DT_PART_MICROSECOND, DT_PART_EPOCH_SECOND, DT_PART_YYYYMM, DT_PART_YYYYMMDD,
 DT_PART_YYYYMMDDHH, DT_PART_YYYYMMDDHHMMSS, DT_PART_DATE) = range(19)
DT_UNIT_YEAR, DT_UNIT_QUARTER, DT_UNIT_MONTH, DT_UNIT_WEEK, DT_UNIT_DAY, DT_UNIT_HOUR, DT_UNIT_MINUTE, DT_UNIT_SECOND = range(8)
DT_WEEK_SUNDAY = 1

# dbhip_str_slice_op, dbhip_str_build_op and the flag of dbhip_str_length / dbhip_str_slice
STR_SUBSTR, STR_LEFT, STR_RIGHT, STR_TRIM_LEADING, STR_TRIM_TRAILING, STR_TRIM_BOTH = range(6)
STR_CONCAT, STR_UPPER, STR_LOWER = range(3)
STR_UNIT_BYTE = 1

# the flag of dbhip_inlist_eval, dbhip_inlist_path_t and the limits of dbhip_inlist_create
IN_NEGATE = 1
IN_PATH_BITS, IN_PATH_COMPARE, IN_PATH_TABLE = range(3)
IN_MAX_ITEMS, IN_MAX_ITEM_BYTES, IN_MAX_LONG_BYTES = 1024, 255, 16384

# the create flags of dbhip_regex_check / dbhip_regex_create, the flag of dbhip_regex_eval and the limits of the group
REGEX_CASE_INSENSITIVE, REGEX_DOT_NL, REGEX_UNIT_BYTE, REGEX_FULL_MATCH = 1, 2, 4, 8
REGEX_NEGATE = 1
REGEX_MAX_PATTERN, REGEX_MAX_STATES, REGEX_MAX_TABLE_BYTES = 1024, 4096, 32768

# DBHIP_STR_PARSE_MAX_BYTES: dbhip_str_parse declines a longer value unread
STR_PARSE_MAX_BYTES = 256

# dbhip_str_rewrite_op (the flag of the group is STR_UNIT_BYTE)
STRW_REPLACE, STRW_LPAD, STRW_RPAD, STRW_REPEAT, STRW_REVERSE = range(5)

# dbhip_array_reduce_kind, dbhip_array_find_op and the limits of the group (DBHIP_ARRAY_LONG_LEN; csrc/dev_array.h's stage and needle)
ARR_COUNT, ARR_SUM, ARR_MIN, ARR_MAX = range(4)
ARR_CONTAINS, ARR_INDEXOF = range(2)
ARRAY_LONG_LEN, ARRAY_STAGE_BYTES, ARRAY_MAX_NEEDLE = 32, 8192, 255

# dbhip_math_fn
MATH_ABS, MATH_SIGN, MATH_CEIL, MATH_FLOOR, MATH_ROUND, MATH_TRUNCATE, MATH_SQRT = range(7)

# dbhip_bool_op and DBHIP_CASE_MAX_CONDS
BOOL_AND, BOOL_OR, BOOL_NOT, BOOL_XOR = range(4)
CASE_MAX_CONDS = 16


def library_path():
    # DBHIP_LIBRARY: another build of the same library (same-box A/B runs against an older commit's build)
    return os.environ.get("DBHIP_LIBRARY") or os.path.join(_HERE, "libdbhip.so")


# every symbol include/dbhip.h declares (tests check that the built library exports all of them)
SYMBOLS = [
    "dbhip_abi_version", "dbhip_init", "dbhip_device_count", "dbhip_last_error", "dbhip_alloc", "dbhip_free", "dbhip_trim",
    "dbhip_memcpy_h2d", "dbhip_memcpy_d2h", "dbhip_memset", "dbhip_stream_create", "dbhip_stream_destroy", "dbhip_stream_release_scratch", "dbhip_stream_cancel", "dbhip_stream_cancel_clear",
    "dbhip_stream_sync", "dbhip_event_create", "dbhip_event_record", "dbhip_event_elapsed_ms",
    "dbhip_event_destroy", "dbhip_last_kernel_ms", "dbhip_arith", "dbhip_arith_result_type", "dbhip_sum_a_plus_b_mul_c_i64",
    "dbhip_sum", "dbhip_expr_eval", "dbhip_decimal_result_size", "dbhip_decimal_arith", "dbhip_decimal_neg", "dbhip_decimal_cast", "dbhip_cmp", "dbhip_bitmap_binary",
    "dbhip_bitmap_count", "dbhip_filter_select", "dbhip_select_cmp", "dbhip_select_bool", "dbhip_take", "dbhip_take_block", "dbhip_take_bitmap", "dbhip_group_hash",
    "dbhip_groupby_create", "dbhip_groupby_add_block", "dbhip_groupby_merge_serialized", "dbhip_groupby_merge_state_block",
    "dbhip_groupby_num_groups", "dbhip_groupby_row_bytes", "dbhip_groupby_flush_serialized", "dbhip_groupby_flush_block",
    "dbhip_groupby_merge_blocks", "dbhip_groupby_add_block_filtered", "dbhip_groupby_partition_blocks",
    "dbhip_groupby_replace_with_blocks", "dbhip_groupby_flush_partitioned", "dbhip_groupby_flush_result_nullable",
    "dbhip_groupby_state_fields", "dbhip_groupby_flush_state_block", "dbhip_groupby_add_block_program", "dbhip_groupby_prepare_program", "dbhip_groupby_set_pipelined", "dbhip_groupby_checkpoint", "dbhip_groupby_arena", "dbhip_groupby_merge_serialized_arena", "dbhip_sel_from_ranges", "dbhip_sel_from_repeats", "dbhip_take_chunks", "dbhip_take_outer", "dbhip_cast", "dbhip_memcpy_d2d",
    "dbhip_groupby_result_type", "dbhip_groupby_flush_result", "dbhip_groupby_reset",
    "dbhip_groupby_destroy", "dbhip_q1_create_groupby", "dbhip_q1_fused", "dbhip_keys_method", "dbhip_pack_keys", "dbhip_serialize_keys_offsets", "dbhip_serialize_keys", "dbhip_join_create_binary",
    "dbhip_join_add_build_binary", "dbhip_join_finalize_binary", "dbhip_join_probe_count_binary", "dbhip_join_probe_binary", "dbhip_join_destroy_binary",
    "dbhip_join_create", "dbhip_join_create_keys", "dbhip_join_probe_mark",
    "dbhip_join_add_build", "dbhip_join_finalize", "dbhip_join_probe_count", "dbhip_join_probe",
    "dbhip_join_destroy", "dbhip_join_mark_build", "dbhip_join_build_matched", "dbhip_sort_perm", "dbhip_merge_sorted_perm", "dbhip_sort_bound_partition",
    "dbhip_window_bounds", "dbhip_window_rank", "dbhip_window_shift", "dbhip_window_value", "dbhip_window_aggregate",
    "dbhip_like_kind", "dbhip_like", "dbhip_str_match", "dbhip_dt_part_type", "dbhip_dt_part", "dbhip_dt_trunc", "dbhip_dt_add", "dbhip_dt_diff", "dbhip_str_length", "dbhip_str_slice", "dbhip_str_build_bytes", "dbhip_str_build",
    "dbhip_inlist_create", "dbhip_inlist_path", "dbhip_inlist_eval", "dbhip_inlist_destroy", "dbhip_str_parse", "dbhip_str_format_bytes", "dbhip_str_format", "dbhip_regex_check", "dbhip_regex_create", "dbhip_regex_eval", "dbhip_regex_destroy", "dbhip_math_result", "dbhip_math", "dbhip_case_check", "dbhip_case", "dbhip_coalesce", "dbhip_bool_logic",
    "dbhip_str_position", "dbhip_str_split_part", "dbhip_str_rewrite_bytes", "dbhip_str_rewrite",
    "dbhip_array_length", "dbhip_array_get", "dbhip_array_find", "dbhip_array_find_str", "dbhip_array_reduce_result", "dbhip_array_reduce", "dbhip_array_unnest_sel",
    "dbhip_bitmap_set_indices", "dbhip_siphash64", "dbhip_scatter_indices", "dbhip_scatter_block", "dbhip_vec_distance", "dbhip_vec_distance_rows", "dbhip_vec_topk", "dbhip_score_u8",
    "dbhip_vec_topk_merge", "dbhip_vec_index_build", "dbhip_vec_index_search", "dbhip_vec_index_destroy",
    "dbhip_comm_unique_id", "dbhip_comm_create", "dbhip_comm_destroy", "dbhip_comm_abort", "dbhip_comm_allgather", "dbhip_comm_alltoall",
    "dbhip_comm_allreduce_sum_u64", "dbhip_groupby_exchange_allgather", "dbhip_groupby_exchange_alltoall", "dbhip_kmeans", "dbhip_vec_kernel_f32", "dbhip_hnsw_build", "dbhip_hnsw_build_sequential", "dbhip_hnsw_from_graph", "dbhip_hnsw_open", "dbhip_hnsw_export_graph", "dbhip_hnsw_search", "dbhip_hnsw_scores",
    "dbhip_hnsw_encoded", "dbhip_hnsw_meta", "dbhip_hnsw_destroy",
    "dbhip_pq_chunk_open", "dbhip_pq_chunk_validity", "dbhip_pq_chunk_image", "dbhip_pq_chunk_decode", "dbhip_pq_chunk_close",
    "dbhip_pq_chunk_open_device", "dbhip_pq_chunk_decode_device", "dbhip_pq_chunks_decode_device", "dbhip_pq_chunk_open_device_list", "dbhip_pq_chunk_decode_device_list",
    "dbhip_pq_chunk_take_arena", "dbhip_pq_chunk_open_device_nested", "dbhip_pq_chunk_decode_device_nested",
    "dbhip_scatter_columns", "dbhip_concat_columns", "dbhip_comm_create_loopback", "dbhip_exchange_begin", "dbhip_shuffle_exchange_begin", "dbhip_sort_exchange_begin", "dbhip_exchange_finish", "dbhip_exchange_string_bytes", "dbhip_exchange_finish_strings", "dbhip_exchange_destroy", "dbhip_vec_topk_allgather",
    # diagnostics and test hooks (declared in the header's last section)
    "dbhip_groupby_debug_set_hash_mask", "dbhip_groupby_debug_set_partition_bits", "dbhip_groupby_debug_set_compact", "dbhip_join_binary_debug_set_hash_mask",
    "dbhip_fagg_stats", "dbhip_scratch_stats", "dbhip_jit_compile_check", "dbhip_jit_offline",
]
_RESTYPE_I64 = {"dbhip_jit_compile_check", "dbhip_jit_offline"}


def load_library():
    """dlopen libdbhip.so (no GPU needed to load; compute entry points need one)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise DbhipError(ERR_NO_DEVICE, f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                       "(there is no CPU fallback)")
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    L.dbhip_last_error.restype = C.c_char_p
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name != "dbhip_last_error":
            fn.restype = C.c_int64 if name in _RESTYPE_I64 else C.c_int32
    # the LIKE group: (pattern, len, escape) / (col, pattern, len, escape, flags, n, out, stream) / (kind, col, needle, len, flags, n, out, stream)
    L.dbhip_like_kind.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.dbhip_like.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_match.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    # the Date / Timestamp group: (part, col, tz, n, out, stream) / (unit, flags, col, out_type, tz, n, out, stream) /
    # (unit, col, delta, tz, n, out, err_bitmap, err_count, stream) / (unit, a, b, tz, n, out, stream)
    L.dbhip_dt_part_type.argtypes = [C.c_int32, C.c_int32]
    L.dbhip_dt_part.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_dt_trunc.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_dt_add.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_dt_diff.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    # the String function group: (col, flags, n, out, stream) / (op, col, a, b, pad, pad_len, flags, n, out_views, stream) /
    # (op, args, nargs, n, out_bytes_host, stream) / (op, args, nargs, n, out_views, out_data, out_data_bytes, out_validity, err_count,
    # non_ascii_count, stream)
    L.dbhip_str_length.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_slice.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_build_bytes.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_build.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # the IN-list group: (type, precision, scale, values, offsets, n_items, has_null, out) / (set) / (set, col, flags, n, out_bitmap,
    # out_validity, stream) / (set)
    L.dbhip_inlist_create.argtypes = [C.c_int32, C.c_uint8, C.c_uint8, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.dbhip_inlist_path.argtypes = [C.c_void_p]
    L.dbhip_inlist_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_inlist_destroy.argtypes = [C.c_void_p]
    # the regular-expression group: (pattern, len, flags, out_info[4]) / (pattern, len, flags, out) / (handle, col, flags, n, out_bitmap,
    # out_declined, declined_count, stream) / (handle)
    L.dbhip_regex_check.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.dbhip_regex_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.dbhip_regex_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_regex_destroy.argtypes = [C.c_void_p]
    # the String cast group: (src, dst_type, precision, scale, is_try, rounding_mode, offset_s, n, out, bitmap, err_count, declined_count,
    # stream) / (src, offset_s, n, out_bytes_host, stream) / (src, offset_s, n, out_views, out_data, out_data_bytes, err_count, stream)
    L.dbhip_str_parse.argtypes = [C.c_void_p, C.c_int32, C.c_uint8, C.c_uint8, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]
    L.dbhip_str_format_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_format.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    # String search and rewrite: (col, needle, len, start, flags, n, out, stream) / (col, delim, len, part, n, out_views, stream) /
    # (op, col, k, x, x_len, y, y_len, flags, n, out_bytes_host, stream) / (op, col, k, x, x_len, y, y_len, flags, n, out_views, out_data,
    # out_data_bytes, err_count, stream)
    L.dbhip_str_position.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_split_part.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_rewrite_bytes.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.dbhip_str_rewrite.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_uint64, C.c_void_p, C.c_void_p]
    # the Array group: (offsets, n, n_elems, out, bad_rows, stream) / (elems, offsets, n, n_elems, index, out_values, out_validity, stream) /
    # (op, elems, offsets, n, n_elems, needle, out, stream) / (op, elems, offsets, n, n_elems, needle, len, out, stream) /
    # (kind, elem_type, precision, scale, out_type, out_precision, out_scale) / (kind, elems, offsets, n, n_elems, out, out_validity,
    # err_count, stream) / (offsets, n, n_elems, out_sel, num_out, stream)
    L.dbhip_array_length.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_array_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_array_find.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_array_find_str.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.dbhip_array_reduce_result.argtypes = [C.c_int32, C.c_int32, C.c_uint8, C.c_uint8, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_array_reduce.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_array_unnest_sel.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p]
    # the math group: (fn, src_type, src_precision, src_scale, digits, out_type, out_precision, out_scale) / (fn, src, digits, n, out, stream)
    L.dbhip_math_result.argtypes = [C.c_int32, C.c_int32, C.c_uint8, C.c_uint8, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_math.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    # the conditionals: (conds, n_conds, values, n_values) / (conds, n_conds, values, n, out, out_validity, out_branch, out_buffers,
    # out_n_buffers, stream) / (args, n_args, n, out, out_validity, out_branch, out_buffers, out_n_buffers, stream) /
    # (op, a, b, n, out_values, out_validity, stream)
    L.dbhip_case_check.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    L.dbhip_case.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_coalesce.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dbhip_bool_logic.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    _LIB = L
    return L


def lib():
    return load_library()


def check(rc):
    if rc != OK:
        raise DbhipError(rc, load_library().dbhip_last_error().decode("utf-8", "replace"))
    return rc
