"""ctypes binding of libdrandhip.so (the product library).

The library is built in-tree by `make -C drand_amd` (or __graft_entry__.build()). There is no CPU
fallback: if the library or the GPU is missing, calls raise. The CPU oracle under oracle/ is test
infrastructure and is never imported here.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DRANDHIP_LIB") or os.path.join(HERE, "libdrandhip.so")

DH_OK = 0
DH_EINVAL = -1
DH_EDEVICE = -2
DH_ENOMEM = -3
DH_EKEY = -4
DH_ERECOVER = -5
DH_EBUSY = -6
DH_EABANDONED = -7
DH_ECORRUPT = -8
DH_ENOBEACON = -9
DH_NODE_CHECKED = 2
DH_DEFERRED = 1
DH_STORE_TRIMMED, DH_STORE_UNTRIMMED, DH_STORE_AUTO = 0, 1, 2
DH_PATCH_DELETE = 0xFFFFFFFF
DH_AR_DEFERRED, DH_AR_NO_SIGNATURE, DH_AR_INVALID, DH_AR_RANDOMNESS = 1, 2, 4, 8
DH_AR_SEQUENCE, DH_AR_LINK, DH_AR_PRED_DEFERRED = 16, 32, 64
DH_AR_BEACON_ID = 128
DH_PB_BEACON_PACKET, DH_PB_PUBLIC_RAND = 1, 2
DH_ENC_RANDOM_DATA_JSON, DH_ENC_PUBLIC_RAND_PB = 1, 2
DH_ENC_NEWLINE, DH_ENC_DELIMITED = 1, 2
DH_AS_CHOSEN, DH_AS_DUPLICATE, DH_AS_INVALID, DH_AS_STALE, DH_AS_SKIPPED, DH_AS_CONFLICT = 1, 2, 4, 8, 16, 32
DH_AS_GAP, DH_AS_LINK = 1, 2

# every symbol declared in include/drandhip.h, with (restype, argtypes)
_c = ctypes
_P = _c.c_void_p
SIGNATURES = {
    "dh_init": (_c.c_int, [_c.c_uint32]),
    "dh_shutdown": (None, []),
    "dh_scheme_from_name": (_c.c_int, [_c.c_char_p]),
    "dh_sig_len": (_c.c_int, [_c.c_int]),
    "dh_key_len": (_c.c_int, [_c.c_int]),
    "dh_verify_batch": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P,
                                   _c.c_size_t, _P, _P, _c.c_uint64]),
    "dh_verify_batch_device": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _P, _P, _c.c_size_t, _P, _c.c_size_t,
                                          _P, _c.c_size_t, _P, _P, _c.c_uint64, _P, _P]),
    "dh_verify_beacon": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _c.c_uint64, _c.c_char_p, _c.c_size_t,
                                    _c.c_char_p, _c.c_size_t]),
    "dh_verify_recovered": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _c.c_char_p, _c.c_char_p, _c.c_size_t]),
    "dh_verify_recovered_batch": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _P, _P, _c.c_size_t, _c.c_size_t, _P,
                                             _c.c_uint64]),
    "dh_digest_batch": (_c.c_int, [_c.c_int, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P]),
    "dh_randomness_batch": (_c.c_int, [_c.c_int, _P, _c.c_size_t, _c.c_size_t, _P]),
    "dh_recover_batch": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_int, _c.c_int, _P, _P, _P, _c.c_size_t, _P, _P]),
    "dh_verify_partials_batch": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_int, _c.c_int, _P, _P, _P, _c.c_size_t, _P]),
    "dh_bls_verify_batch": (_c.c_int, [_c.c_int, _P, _c.c_size_t, _P, _P, _P, _P, _c.c_size_t, _c.c_size_t, _P, _P,
                                       _c.c_uint64, _P]),
    "dh_identity_hash_batch": (_c.c_int, [_c.c_int, _P, _c.c_size_t, _P]),
    "dh_identity_verify_batch": (_c.c_int, [_c.c_int, _P, _P, _c.c_size_t, _c.c_size_t, _P]),
    "dh_schnorr_verify_batch": (_c.c_int, [_c.c_int, _P, _c.c_size_t, _P, _P, _P, _P, _c.c_size_t, _c.c_size_t, _P, _P]),
    "dh_schnorr_sig_len": (_c.c_int, [_c.c_int]),
    "dh_sign_batch": (_c.c_int, [_c.c_int, _c.c_char_p, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P]),
    "dh_public_key": (_c.c_int, [_c.c_int, _c.c_char_p, _P]),
    "dh_partial_bytes": (_c.c_int, [_c.c_int]),
    "dh_set_split": (_c.c_int, [_c.c_uint64, _c.c_int]),
    "dh_hash_to_curve": (_c.c_int, [_c.c_int, _P, _P, _c.c_size_t, _c.c_char_p, _c.c_size_t, _P]),
    "dh_g1_round_prep_debug": (_c.c_int, [_P, _P, _c.c_size_t, _P, _P, _P]),
    "dh_g1_round_prep_late_debug": (_c.c_int, [_P, _P, _c.c_size_t, _P, _P, _P]),
    "dh_msm_level0_shape_debug": (_c.c_int, [_P, _P, _P, _P]),
    "dh_field_ops_debug": (_c.c_int, [_P, _P, _c.c_size_t, _c.c_size_t, _P, _c.c_size_t]),
    "dh_vm_debug": (_c.c_int, [_c.c_int, _P, _c.c_size_t, _P, _c.c_size_t, _c.c_size_t, _c.c_size_t, _P, _c.c_size_t,
                               _c.c_size_t, _P, _c.c_size_t]),
    "dh_batch_begin": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P,
                                  _c.c_size_t, _P, _P, _c.c_uint64, _P, _c.POINTER(_P), _P]),
    "dh_batch_check": (_c.c_int, [_P, _P, _c.c_size_t, _P]),
    "dh_batch_stream": (_P, [_P]),
    "dh_check_partials": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _P, _c.c_size_t, _c.POINTER(_c.c_int)]),
    "dh_batch_finish": (_c.c_int, [_P, _c.c_int, _P]),
    "dh_bolt_index": (_c.c_int, [_P, _c.c_size_t, _P, _P, _c.c_size_t, _P]),
    "dh_store_open_bolt": (_c.c_int, [_P, _c.c_size_t, _c.POINTER(_P)]),
    "dh_store_stat": (_c.c_int, [_P, _P]),
    "dh_store_columns_device": (_c.c_int, [_P, _c.c_uint64, _c.c_uint64, _c.c_size_t, _P, _P, _P, _c.c_size_t, _P, _P,
                                           _c.c_size_t, _P, _P]),
    "dh_store_check_past": (_c.c_int, [_P, _c.c_int, _c.c_char_p, _c.c_size_t, _c.c_uint64, _c.c_size_t, _c.c_uint64, _P,
                                       _c.c_size_t, _P, _P, _P]),
    "dh_store_close": (None, [_P]),
    "dh_store_open_bolt_format": (_c.c_int, [_P, _c.c_size_t, _c.c_int, _c.POINTER(_P)]),
    "dh_store_format_stat": (_c.c_int, [_P, _P]),
    "dh_store_beacons_device": (_c.c_int, [_P, _c.c_uint64, _c.c_uint64, _c.c_size_t, _c.c_size_t, _P, _P, _P, _P, _P, _P,
                                           _c.c_size_t, _P, _P, _c.c_size_t, _P, _P]),
    "dh_store_deferred": (_c.c_int, [_P, _c.c_uint64, _c.c_uint64, _P, _c.c_size_t, _P]),
    "dh_bolt_write_trimmed_device": (_c.c_int, [_P, _P, _c.c_size_t, _P, _c.c_size_t, _c.c_uint32, _P, _c.c_size_t, _P, _P, _P]),
    "dh_store_save_trimmed": (_c.c_int, [_P, _c.c_uint64, _c.c_uint64, _P, _P, _c.c_size_t, _P, _c.c_size_t, _c.c_uint32, _P,
                                         _c.c_size_t, _P, _P, _c.c_size_t, _P, _P]),
    "dh_bolt_writer_open": (_c.c_int, [_c.c_uint32, _c.POINTER(_P)]),
    "dh_bolt_writer_append_device": (_c.c_int, [_P, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_size_t, _P, _P, _P, _P]),
    "dh_bolt_writer_finish": (_c.c_int, [_P, _P, _c.c_size_t, _P, _P, _P, _P]),
    "dh_bolt_writer_close": (None, [_P]),
    "dh_store_save_trimmed_append": (_c.c_int, [_P, _P, _c.c_uint64, _c.c_uint64, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P,
                                                _c.c_size_t, _P, _P, _P, _c.c_size_t, _P, _P]),
    "dh_store_split": (_c.c_int, [_P, _c.c_uint64, _c.c_uint64, _c.c_size_t, _P, _c.c_size_t, _P]),
    "dh_archive_open_ndjson": (_c.c_int, [_P, _c.c_size_t, _c.POINTER(_P)]),
    "dh_archive_stat": (_c.c_int, [_P, _P]),
    "dh_archive_lines": (_c.c_int, [_P, _c.c_uint64, _c.c_size_t, _P, _P]),
    "dh_archive_deferred": (_c.c_int, [_P, _c.c_uint64, _c.c_size_t, _P, _c.c_size_t, _P]),
    "dh_archive_beacons_device": (_c.c_int, [_P, _c.c_uint64, _c.c_size_t, _c.c_size_t, _c.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P,
                                             _P, _P]),
    "dh_archive_check": (_c.c_int, [_P, _c.c_int, _c.c_char_p, _c.c_size_t, _c.c_uint64, _c.c_size_t, _P, _P, _c.c_size_t,
                                    _c.c_size_t, _c.c_uint64, _P, _P]),
    "dh_archive_close": (None, [_P]),
    "dh_archive_open_pb": (_c.c_int, [_c.c_int, _P, _c.c_size_t, _P, _P, _c.c_size_t, _c.POINTER(_P)]),
    "dh_archive_kind": (_c.c_int, [_P]),
    "dh_archive_set_beacon_id": (_c.c_int, [_P, _P, _c.c_size_t]),
    "dh_pb_frame_delimited": (_c.c_int, [_P, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P]),
    "dh_pb_encode_device": (_c.c_int, [_c.c_int, _P, _P, _c.c_size_t, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P, _c.c_size_t,
                                       _c.c_int, _P, _c.c_size_t, _P, _P, _P]),
    "dh_rand_encode_device": (_c.c_int, [_c.c_int, _P, _P, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P, _P, _c.c_size_t, _P, _c.c_size_t,
                                         _c.c_int, _P, _c.c_size_t, _P, _P, _P]),
    "dh_assemble_device": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P, _c.c_size_t, _P, _P,
                                      _c.c_size_t, _P, _c.c_size_t, _c.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _c.c_size_t, _P,
                                      _P, _P]),
    "dh_sort_rounds_debug": (_c.c_int, [_P, _c.c_size_t, _P]),
    "dh_profile": (_c.c_int, [_c.c_int]),
    "dh_profile_read": (_c.c_int, [_c.c_char_p, _c.c_size_t]),
    "dh_last_error_string": (_c.c_char_p, []),
    "dh_version": (_c.c_char_p, []),
}

_lib = None


class LibraryMissing(RuntimeError):
    pass


def load():
    """Load libdrandhip.so (no build, no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            "libdrandhip.so not found at %s: build it with `make -C drand_amd` or __graft_entry__.build()" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return (load().dh_last_error_string() or b"").decode()
