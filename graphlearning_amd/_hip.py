"""ctypes binding of libglx.so (include/glx.h): the only way the package reaches the GPU.

There is NO CPU fallback: if the library is missing or no MI355X is visible the calls
raise GlxError.  The library is loaded lazily (first use), so importing the package
never creates HIP state -- safe for the joblib process pools the reference's
ssl_trials uses (reference graphlearning/ssl.py:390-396).
"""
import os
import ctypes as C
import numpy as np

GLX_F32, GLX_F64 = 0, 1
GLX_CG_NP1D, GLX_CG_TREE, GLX_CG_X0, GLX_CG_BLOCKS, GLX_CG_CHAIN, GLX_CG_EAGER = 1, 2, 4, 8, 16, 32     # flags of glx_cg_solve / glx_cg_groups_masked (include/glx.h)
# how reduce='exact' walks numpy's reduction chains: None = the library's choice (block form from 8192 rows on), 'blocks' / 'chain'
# force one form (same bits; tests and measurements)
CG_EXACT_FORM = None
CG_EXACT_EAGER = False          # True: the exact-mode CG enqueues its iterations launch by launch (GLX_CG_EAGER) instead of replaying captured chunks
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libglx.so')
_lib = None
_default_device = int(os.environ.get('GLX_DEVICE', '0'))


def set_default_device(device):
    """GPU used by every call that is not given an explicit `device` (one process per GPU: set it
    to LOCAL_RANK once).  Initial value: $GLX_DEVICE or 0."""
    global _default_device
    _default_device = int(device)


def default_device():
    return _default_device


def _dev(device):
    if device is None:
        return _default_device
    if hasattr(device, 'index') and not isinstance(device, int):     # a torch.device
        return int(device.index or 0)
    return int(device)


class GlxError(RuntimeError):
    pass


def _dt(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return GLX_F32
    if dtype == np.float64:
        return GLX_F64
    raise GlxError('unsupported dtype %s (float32 or float64)' % dtype)


_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p

# name -> (argtypes); every function returns int status unless listed in _SPECIAL
_SIGNATURES = {
    'glx_version': [],
    'glx_device_count': [C.POINTER(C.c_int)],
    'glx_device_synchronize': [],
    'glx_host_alloc': [C.c_size_t, C.POINTER(_vp)],
    'glx_host_free': [_vp],
    'glx_graph_create': [C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_graph_create_resident': [C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)],
    'glx_graph_set_row_transform': [_vp, _vp, C.c_int],
    'glx_graph_destroy': [_vp],
    'glx_graph_info': [_vp, _i64p],
    'glx_graph_order': [_vp, _vp],
    'glx_graph_set_order': [_vp, _vp],
    'glx_spmm_bias': [_vp, _vp, _vp, _vp, C.c_int, C.c_int],
    'glx_poisson_sweep': [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(C.c_int)],
    'glx_sweep_create': [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_sweep_set_problem': [_vp, _vp, _vp, _vp, _vp],
    'glx_sweep_set_vectors': [_vp, _vp, _vp],
    'glx_sweep_set_problem_rows': [_vp, C.c_int64, _vp, _vp, _vp, C.c_double],
    'glx_sweep_run': [_vp, C.POINTER(C.c_int), C.POINTER(C.c_float)],
    'glx_sweep_fetch': [_vp, _vp],
    'glx_sweep_launches': [_vp, _i64p],
    'glx_sweep_stop_values': [_vp, C.c_int64, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'glx_sweep_destroy': [_vp],
    'glx_sweep_set_state': [_vp, _vp, _vp],
    'glx_sweep_set_state_labels': [_vp, _vp, C.c_int64, _vp, _vp],
    'glx_sweep_iterate': [_vp, C.c_int],
    'glx_sweep_groups_create': [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_sweep_groups_set_vectors': [_vp, _vp, _vp],
    'glx_sweep_groups_set_problem_rows': [_vp, C.c_int, C.c_int64, _vp, _vp, _vp, C.c_double],
    'glx_sweep_groups_run': [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)],
    'glx_sweep_groups_stop_values': [_vp, C.c_int, C.c_int64, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'glx_sweep_groups_fetch': [_vp, C.c_int, _vp],
    'glx_sweep_groups_project': [_vp, C.c_int, _vp, _vp, _vp, _f64p, C.POINTER(C.c_int), C.c_int, C.c_int],
    'glx_sweep_groups_launches': [_vp, _i64p],
    'glx_sweep_groups_destroy': [_vp],
    'glx_record_layout': [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)],
    'glx_graph_slots': [_vp, C.c_int, C.c_int, _i64p],
    'glx_bias_flags_dev': [_vp, C.c_int, C.c_int, _vp, _vp, _vp],
    'glx_sweep_step_dev': [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'glx_pack_records_dev': [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp],
    'glx_unpack_records_dev': [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp],
    'glx_rec_dots_dev': [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp],
    'glx_rec_axpy2_dev': [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp],
    'glx_rec_xpby_dev': [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp],
    'glx_dist_unique_id': [_vp],
    'glx_dist_init_rank': [C.c_int, C.c_int, _vp, C.c_int, C.POINTER(_vp)],
    'glx_dist_init': [C.c_int, _vp, C.POINTER(_vp)],
    'glx_dist_comm_info': [_vp, C.POINTER(C.c_int32)],
    'glx_dist_destroy': [_vp],
    'glx_dist_sweep_create': [_vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int64,
                              C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_dist_sweep_set_problem': [_vp, _vp, _vp, _vp, _vp],
    'glx_poisson_sweep_dist': [_vp, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_float)],
    'glx_dist_sweep_fetch': [_vp, _vp],
    'glx_dist_sweep_stats': [_vp, _i64p],
    'glx_dist_sweep_info': [_vp, _i64p],
    'glx_dist_sweep_time_parts': [_vp, C.c_int, _f32p],
    'glx_dist_sweep_destroy': [_vp],
    'glx_dist_sweep_begin': [_vp],
    'glx_dist_sweep_boundary': [_vp, C.c_int],
    'glx_dist_sweep_get_send': [_vp, _vp],
    'glx_dist_sweep_put_halo': [_vp, _vp, C.c_int],
    'glx_dist_sweep_interior': [_vp, C.c_int, _f64p],
    'glx_cg_multi': [_vp, _vp, _vp, C.c_int, C.c_double, C.c_int64, C.POINTER(C.c_int), _f64p],
    'glx_cg_solve': [_vp, _vp, _vp, C.c_int, C.c_double, C.c_int64, C.c_int, C.POINTER(C.c_int), _f64p],
    'glx_sweep_project_iterate': [_vp, _vp, _vp, _vp, _f64p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int],
    'glx_lp_iterate': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_int64, C.c_double, C.c_int64, C.c_int64, C.c_int64,
                       C.POINTER(C.c_int64), C.c_int],
    'glx_affine_iterate': [_vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int64, C.POINTER(C.c_int64), _f64p],
    'glx_cg_groups_masked': [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_int64, C.c_int, C.POINTER(C.c_int), _f64p],
    'glx_cg_groups_rows': [_vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_int64, C.c_int,
                           C.POINTER(C.c_int), _f64p],
    'glx_cg_last_stop_margin': [_vp, _f64p],
    'glx_pool_set_enabled': [C.c_int],
    'glx_pool_set_poison': [C.c_int],
    'glx_debug_set': [C.c_int],
    'glx_debug_counters': [_vp],
    'glx_upload_stats': [_vp],
    'glx_upload_set_mode': [C.c_int],
    'glx_nearest_dist': [_vp, C.c_int64, C.c_int, _vp, C.c_int64, _vp, C.c_int],
    'glx_cg_last_block_stats': [_vp, C.POINTER(C.c_int)],
    'glx_host_fingerprint': [_vp, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64)],
    'glx_knn_search': [_vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_knn_result_lists': [_vp, _vp, _vp],
    'glx_knn_result_order': [_vp, _vp],
    'glx_knn_result_to_csr': [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, C.POINTER(C.c_int64)],
    'glx_knn_result_destroy': [_vp],
    'glx_ball_search': [_vp, C.c_int64, C.c_int, C.c_double, _vp, C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_ball_result_nnz': [_vp, _i64p],
    'glx_ball_result_to_csr': [_vp, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _i64p],
    'glx_ball_result_destroy': [_vp],
    'glx_ball_stats': [_f64p],
    'glx_sssp': [C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int, _vp, _vp, _i64p, _f64p, C.c_int],
    'glx_components': [C.c_int64, C.c_int64, _vp, _vp, _vp, _i64p, _f64p, C.c_int],
    'glx_components_set_wave_row': [C.c_int],
    'glx_components_plan': [_i64p],
    'glx_boundary_stat': [C.c_int64, C.c_int, _vp, C.c_int64, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _f64p, C.c_int],
    'glx_boundary_stat_set_wave_row': [C.c_int],
    'glx_peikonal': [C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int, _vp, C.c_int64, _vp, _i64p, _f64p,
                     C.c_int],
    'glx_lip_iterate': [C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_int, C.c_double, C.c_double, C.c_int64, C.c_double,
                        _vp, _vp, _vp, _vp, C.c_int, C.c_int],
    'glx_slp_iterate': [C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_int],
    'glx_lp_iterate_batch': [C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_double, C.c_int64, C.c_double, _vp, _vp, _vp,
                             C.c_int],
    'glx_ck_solve': [C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int64, _vp, _vp, _vp, C.c_int64, C.c_double, C.c_double, C.c_int64, _vp,
                     _f64p, _i64p, _vp, C.c_int64, _vp, _vp, _vp, C.c_int],
    'glx_dlp_solve': [C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_double, C.c_double, C.c_int64, _vp, _vp, _vp,
                      C.c_int],
    'glx_mmbo_solve': [C.c_int64, C.c_int, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_double, C.c_double, _vp, _vp, _vp,
                       C.c_int],
    'glx_eig_create': [C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_eig_set_column': [_vp, C.c_int, _vp],
    'glx_eig_orthonormalize': [_vp, C.c_int, _f64p],
    'glx_eig_run': [_vp, C.c_int, C.c_int, _vp, _vp],
    'glx_eig_rotate': [_vp, _vp, C.c_int, C.c_int],
    'glx_eig_get_columns': [_vp, C.c_int, C.c_int, _vp],
    'glx_eig_destroy': [_vp],
    'glx_incres_set_options': [_vp],
    'glx_incres_create': [C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)],
    'glx_incres_step': [_vp, _vp, C.c_int64, C.c_int64, _vp, _i64p],
    'glx_incres_stats': [_vp, _i64p],
    'glx_incres_destroy': [_vp],
    'glx_host_group_by_label': [C.c_int64, _vp, C.c_int, _vp, _vp],
    'glx_acq_create': [C.c_int64, C.c_int, _vp, _vp, C.c_double, C.c_int, C.POINTER(_vp)],
    'glx_acq_compute': [_vp, C.c_int, _vp, C.c_int64, _vp, _vp],
    'glx_acq_update': [_vp, _vp, C.c_int64],
    'glx_acq_greedy': [_vp, C.c_int, _vp, C.c_int64, C.c_int64, _vp, _vp],
    'glx_acq_get_c': [_vp, _vp],
    'glx_acq_stats': [_vp, _i64p],
    'glx_acq_destroy': [_vp],
    'glx_exp_cr': [_vp, _vp, C.c_int64, C.c_int],
    'glx_argmax_project': [_vp, C.c_int64, C.c_int, _vp, _vp, _vp, _f64p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int],
    'glx_argmax_project_t': [_vp, C.c_int, C.c_int64, C.c_int, _vp, _vp, _vp, _f64p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int],
    'glx_knn_bruteforce': [_vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int],
    'glx_knn_bruteforce_range': [_vp, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.c_int],
    'glx_knn_cells_range': [_vp, C.c_int64, C.c_int, C.c_int, _vp, C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.c_int],
    'glx_knn_clustered': [_vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int],
    'glx_knn_set_options': [_vp],
    'glx_knn_stats': [_f64p],
    'glx_knn_to_csr': [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_vp),
                       C.POINTER(_vp), _i64p, C.c_int],
    'glx_knn_rows_to_csr': [_vp, _vp, C.c_int64, C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_int64, C.c_int, C.c_int64, _vp, _vp, _vp,
                            _i64p, C.c_int],
    'glx_host_locality_order': [C.c_int64, _vp, _vp, C.c_int64, _vp],
    'glx_host_permute_rows': [C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'glx_host_row_sums': [C.c_int64, _vp, _vp, _vp],
    'glx_host_neg_columns_rows': [C.c_int64, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int, _vp, C.c_int64, _vp, _vp, _i64p],
    'glx_host_reverse_scale_rows': [C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp],
    'glx_knn_to_csr_into': [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, _i64p, C.c_int],
}
_SPECIAL = {'glx_last_error': ([], C.c_char_p), 'glx_free': ([_vp], None), 'glx_rec_dots_scratch': ([C.c_int64, C.c_int], C.c_int64)}

EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + list(_SPECIAL))


def load(required=True):
    """Load libglx.so (once).  Raises GlxError when it is absent -- build it with
    `python -m graphlearning_amd._build` or `__graft_entry__.build()`."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if required:
            raise GlxError('libglx.so not found at %s: the HIP extension is not built '
                           '(python -m graphlearning_amd._build). There is no CPU fallback.' % LIB_PATH)
        return None
    lib = C.CDLL(LIB_PATH)
    for name, args in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    for name, (args, res) in _SPECIAL.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().glx_last_error()
        raise GlxError('%s failed (%d): %s' % (what or 'libglx call', rc, msg.decode() if msg else '?'))


def call(name, *args):
    """The library function `name` on `args`; a non-zero status raises GlxError with that name and the library's message."""
    check(getattr(load(), name)(*args), name)


def device_count():
    n = C.c_int(0)
    call('glx_device_count', C.byref(n))
    return n.value


def require_device():
    try:
        n = device_count()
    except GlxError as e:
        raise GlxError('no usable HIP device: %s' % e)
    if n < 1:
        raise GlxError('no HIP device visible; graphlearning_amd has no CPU fallback')
    return n


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _dense(a, dtype, shape=None, name='array'):
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise GlxError('%s has shape %s, expected %s' % (name, a.shape, tuple(shape)))
    return a


class _PinnedBlock:
    """A page-locked host block serving as the memory of one numpy array (its `base`); returned to the pool
    when the array and every view of it are gone."""

    def __init__(self, pool, ptr, nbytes, shape, dtype):
        self._pool, self._ptr, self._nbytes = pool, ptr, nbytes
        self.__array_interface__ = {'data': (ptr, False), 'shape': tuple(shape), 'typestr': np.dtype(dtype).str, 'version': 3}

    def __del__(self):
        try:
            self._pool._release(self._ptr, self._nbytes)
        except Exception:
            pass


class _PinnedPool:
    """Result arrays (prob, labels) are handed out as numpy arrays backed by page-locked memory: the device-to-host
    copy then runs at PCIe speed and a fresh array costs no page faults (a 5.6 MB np.empty + first write is ~1 ms).
    Blocks are recycled by size; at most `keep` idle blocks per size are retained.  Page-locked memory cannot be swapped:
    the pool never holds more than `budget` bytes (live arrays + idle blocks; $GLX_PINNED_MAX_MB, default 4096 MiB) --
    beyond it arrays come from ordinary memory, and idle blocks are released first when a request would not fit."""

    def __init__(self, keep=4):
        import threading
        self.keep = keep
        self.idle = {}
        self.total = 0                                   # bytes of page-locked memory this pool currently owns
        self.budget = int(float(os.environ.get('GLX_PINNED_MAX_MB', '4096')) * (1 << 20))
        self.lock = threading.RLock()                    # graphs are built from several Python threads (and by pinned_reserve's helpers)

    def _trim(self):
        for nbytes, lst in list(self.idle.items()):
            while lst:
                ptr = lst.pop()
                self.total -= nbytes
                if _lib is not None:
                    _lib.glx_host_free(_vp(ptr))

    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = max(int(np.prod(shape)) * dtype.itemsize, 1)
        if nbytes < (1 << 16):
            return np.empty(shape, dtype=dtype)
        with self.lock:
            lst = self.idle.get(nbytes)
            ptr = lst.pop() if lst else None
            if ptr is None:
                if self.total + nbytes > self.budget:
                    self._trim()
                if self.total + nbytes > self.budget:
                    return np.empty(shape, dtype=dtype)      # over the budget: ordinary (pageable) memory
                self.total += nbytes                          # (reserved before the allocation: the budget holds across threads)
        if ptr is None:
            p = _vp()
            try:
                call('glx_host_alloc', nbytes, C.byref(p))
            except BaseException:
                with self.lock:
                    self.total -= nbytes
                raise
            ptr = p.value
        return np.asarray(_PinnedBlock(self, ptr, nbytes, shape, dtype))

    def _release(self, ptr, nbytes):
        with self.lock:
            lst = self.idle.setdefault(nbytes, [])
            if len(lst) < self.keep:
                lst.append(ptr)
                return
            self.total -= nbytes
        if _lib is not None:
            _lib.glx_host_free(_vp(ptr))


_pinned = _PinnedPool()

# Off switches of the two buffer pools (results are identical either way: tests/test_gpu_switches.py; the randomised soak runs with
# each off as an ablation -- a result that moves with a switch names the subsystem):
#   PINNED_RESULTS = False   result arrays come from np.empty (ordinary memory), no page-locked block is recycled
#   pool_set_enabled(False)  device work buffers and work sets come straight from / go straight back to the HIP runtime
PINNED_RESULTS = True


def pool_set_enabled(enabled):
    call('glx_pool_set_enabled', 1 if enabled else 0)


def debug_set(flags):
    call('glx_debug_set', int(flags))


def debug_counters():
    out = (C.c_uint64 * 4)()
    call('glx_debug_counters', out)
    return dict(uploads_checked=int(out[0]), engine_readback_differs=int(out[1]), kernel_readback_differs=int(out[2]), bytes_differing=int(out[3]))


def upload_set_mode(mode):
    """0 staged + checked (default), 1 staged, 2 straight from the caller's pageable memory (rounds 1-5)."""
    call('glx_upload_set_mode', int(mode))


def upload_stats():
    """The checked uploads of this process: how many were checked, how many arrived with a wrong sum, how many of those were repaired by a
    repeat, how many given up (glx_upload_stats)."""
    out = (C.c_uint64 * 4)()
    call('glx_upload_stats', out)
    return dict(checked=int(out[0]), wrong_sums=int(out[1]), repaired=int(out[2]), given_up=int(out[3]))


def pool_set_poison(byte):
    """Debugging aid: work buffers are filled with `byte` (0 .. 255) when handed out; None / -1 switches it off."""
    call('glx_pool_set_poison', -1 if byte is None else int(byte))


def pinned_empty(shape, dtype):
    if not PINNED_RESULTS:
        return np.empty(shape, dtype=np.dtype(dtype))
    return _pinned.empty(shape, dtype)


def pinned_reserve(specs):
    """Make sure the pool holds an idle block for every (shape, dtype) of `specs`, allocating the missing ones on a helper thread
    (page-locking 19 MB of fresh memory takes 3.4 ms: weightmatrix.knn starts it beside its search, whose result arrays these
    are).  Returns the thread to join, or None when nothing had to be allocated (the steady state)."""
    need = []
    for shape, dtype in specs if PINNED_RESULTS else ():
        nbytes = max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 1)
        with _pinned.lock:
            if nbytes >= (1 << 16) and not _pinned.idle.get(nbytes) and _pinned.total + nbytes <= _pinned.budget:
                _pinned.total += nbytes              # reserved now, handed to the idle list by the helper
                need.append(nbytes)
    if not need:
        return None
    lib = load()

    def work(nbytes):
        p = _vp()
        ok = lib.glx_host_alloc(nbytes, C.byref(p)) == 0
        with _pinned.lock:
            if ok:
                _pinned.idle.setdefault(nbytes, []).append(p.value)
            else:
                _pinned.total -= nbytes
    import threading
    ths = [threading.Thread(target=work, args=(nb,), daemon=True) for nb in sorted(need, reverse=True)]   # (one per block: page-locking runs in parallel)
    for th in ths:
        th.start()

    class _Join:
        def join(self):
            for th in ths:
                th.join()
    return _Join()


# Communicators and distributed sweeps that are still open when the interpreter shuts down are ABANDONED, not destroyed:
# tearing an RCCL communicator (or the streams and captured graphs that carry its kernels) down from a garbage-collection
# pass during interpreter finalisation was seen to hang the process (a failed test that never reached close(), round 3);
# the operating system reclaims everything at exit anyway.  close() during normal operation destroys as before.
import atexit
import weakref
_abandoned_at_exit = weakref.WeakSet()      # the open objects of the classes that set `_abandon_at_exit`


def _abandon_dist_objects():
    for obj in list(_abandoned_at_exit):
        try:
            obj._h = _vp()
        except Exception:
            pass


atexit.register(_abandon_dist_objects)


class _Handle:
    """Owner of one object of the library: the handle `_h`, opened by the create function a subclass names in `_open` and
    destroyed by the function the subclass names in `_destroy`.  A context manager; close() may be called twice, and every
    later use is refused with GlxError before the library is entered."""

    _destroy = None                 # name of the library function that takes the handle back
    _abandon_at_exit = False        # True: an object still open at interpreter exit is left to the operating system (above)

    def _open(self, name, *args):
        """Create function `name` on `args`; its last parameter, the handle it hands out, is added here."""
        self._h = _vp()
        call(name, *args, C.byref(self._h))
        if self._abandon_at_exit:
            _abandoned_at_exit.add(self)

    def _handle(self):
        if not self._h.value:
            raise GlxError('%s: the object is closed' % type(self).__name__)
        return self._h

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            lib = load(required=False)
            if lib is not None:
                getattr(lib, self._destroy)(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceGraph(_Handle):
    """A sparse operator resident in HBM (glx_graph).  `A` is any scipy sparse matrix;
    the CSR entry order is preserved (see include/glx.h)."""

    _destroy = 'glx_graph_destroy'

    def __init__(self, A, dtype=np.float64, device=None, shape=None, keep_order=False, order=None):
        from scipy import sparse
        A = sparse.csr_matrix(A)
        self.dtype = np.dtype(dtype)
        self.shape = A.shape if shape is None else shape
        self.nnz = int(A.nnz)
        self.device = device = _dev(device)
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        self._open('glx_graph_create', self.shape[0], self.shape[1], self.nnz, _ptr(rowptr), _ptr(col), _ptr(val), _dt(self.dtype), device)
        self._set_order(order, keep_order)

    def _set_order(self, order, keep_order):
        if order is not None:       # the caller's locality order (perm[new] = old) instead of the library's pass over the graph
            perm = np.ascontiguousarray(order, dtype=np.int32)
            if perm.shape != (self.shape[0],):
                raise GlxError('order must be a permutation of the %d rows' % self.shape[0])
            call('glx_graph_set_order', self._handle(), _ptr(perm))
        elif keep_order:
            call('glx_graph_set_order', self._handle(), None)

    @classmethod
    def resident(cls, A, dtype=np.float64, device=None, keep_order=False, order=None, want_row_sums=False):
        """The operator of CSR matrix `A` with the arrays kept on the device only (glx_graph_create_resident); with
        want_row_sums also `A * ones` (scipy's csr_matvec order) computed there: returns (graph, row_sums or None).
        `set_row_transform` then turns the rows into what the operator really is (P = D^-1 W^T: reversed rows times 1 / degree)."""
        self = cls.__new__(cls)
        self.dtype = np.dtype(dtype)
        self.shape = A.shape
        self.nnz = int(A.nnz)
        self.device = device = _dev(device)
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        sums = np.empty(self.shape[0], dtype=np.float64) if want_row_sums else None
        self._open('glx_graph_create_resident', self.shape[0], self.shape[1], self.nnz, _ptr(rowptr), _ptr(col), _ptr(val), _dt(self.dtype), device,
                   _ptr(sums))
        self._set_order(order, keep_order)
        return self, sums

    def set_row_transform(self, row_scale=None, reverse_rows=False):
        sc = None if row_scale is None else _dense(row_scale, np.float64, (self.shape[0],), 'row_scale')
        call('glx_graph_set_row_transform', self._handle(), _ptr(sc), 1 if reverse_rows else 0)

    def info(self):
        out = (C.c_int64 * 8)()
        call('glx_graph_info', self._handle(), out)
        keys = ['n_rows', 'n_cols', 'nnz', 'stored', 'slices', 'rows_per_slice', 'max_row', 'renumbered']
        return dict(zip(keys, list(out)[:8]))

    def order(self):
        """perm[new] = caller's row: the vertex order the library keeps its records in."""
        perm = np.empty(self.shape[0], dtype=np.int32)
        call('glx_graph_order', self._handle(), _ptr(perm))
        return perm

    def spmm_bias(self, u, Db=None, iters=1):
        """`iters` applications of u <- Db + A u (host arrays in, host array out)."""
        u = np.ascontiguousarray(u, dtype=self.dtype)
        if u.ndim == 1:
            return self.spmm_bias(u[:, None], None if Db is None else np.asarray(Db)[:, None], iters)[:, 0]
        if u.shape[0] != self.shape[1]:
            raise GlxError('operand has %d rows, operator has %d columns' % (u.shape[0], self.shape[1]))
        Cc = u.shape[1]
        Dbc = None if Db is None else _dense(Db, self.dtype, (self.shape[0], Cc), 'Db')
        out = np.empty((self.shape[0], Cc), dtype=self.dtype)
        call('glx_spmm_bias', self._handle(), _ptr(Dbc), _ptr(u), _ptr(out), Cc, iters)
        return out

    def poisson_sweep(self, Db, w0, deg, vinf, min_iter=50, max_iter=1000):
        Db = np.ascontiguousarray(Db, dtype=self.dtype)
        n, Cc = Db.shape
        w0 = _dense(w0, np.float64, (n,), 'w0')
        deg = _dense(deg, np.float64, (n,), 'deg')
        vinf = _dense(vinf, np.float64, (n,), 'vinf')
        out = np.empty((n, Cc), dtype=self.dtype)
        T = C.c_int(0)
        call('glx_poisson_sweep', self._handle(), _ptr(Db), _ptr(w0), _ptr(deg), _ptr(vinf), Cc, min_iter, max_iter, _ptr(out), C.byref(T))
        return out, T.value

    def cg(self, B, tol=1e-10, max_iter=100000, x0=None, reduce='exact'):
        """utils.conjgrad on device: returns (X, iterations, err).  x0: initial iterate (B must then
        be the residual b - A@x0, utils.py:510-514).  reduce='tree': tolerance mode (GLX_CG_TREE)."""
        B = np.ascontiguousarray(B, dtype=self.dtype)
        squeeze = B.ndim == 1
        if squeeze:
            B = B[:, None]
        # (a single column, 1-D or (n,1): numpy's axis-0 reduction of it is one contiguous run, summed pairwise)
        flags = (GLX_CG_NP1D if B.shape[1] == 1 else 0) | _reduce_flag(reduce)
        if x0 is None:
            X = np.empty_like(B)
        else:
            X = np.array(np.asarray(x0).reshape(B.shape), dtype=self.dtype, order='C', copy=True)
            flags |= GLX_CG_X0
        it = C.c_int(0)
        err = C.c_double(0)
        call('glx_cg_solve', self._handle(), _ptr(B), _ptr(X), B.shape[1], float(tol), int(max_iter), flags, C.byref(it), C.byref(err))
        return (X[:, 0] if squeeze else X), it.value, err.value

    def affine_iterate(self, u0, b=None, tol=1e-10, max_iter=1000000):
        """u <- A u + b from u0 until max|u_new - u_old| <= tol (graph.page_rank's power iteration):
        returns (u, sweeps, err)."""
        u0 = np.ascontiguousarray(u0, dtype=self.dtype)
        squeeze = u0.ndim == 1
        if squeeze:
            u0 = u0[:, None]
        if b is not None:
            b = np.ascontiguousarray(b, dtype=self.dtype).reshape(u0.shape)
        out = np.empty_like(u0)
        it = C.c_int64(0)
        err = C.c_double(0)
        call('glx_affine_iterate', self._handle(), _ptr(b) if b is not None else None, _ptr(u0), _ptr(out), u0.shape[1], float(tol), int(max_iter),
             C.byref(it), C.byref(err))
        return (out[:, 0] if squeeze else out), it.value, err.value

    def cg_groups(self, B, group_cols, tol=1e-10, max_iter=100000, masks=None, reduce='exact'):
        """Independent systems side by side (columns in groups of `group_cols`), each with its own
        stop test: returns (X, iterations per group, err per group).  masks: per group an array of
        Dirichlet rows (x held at zero there; B is zeroed on them) -- the sub-matrix solve of
        ssl.laplace on the full operator."""
        B = np.ascontiguousarray(B, dtype=self.dtype)
        if masks is not None:
            B = B.copy()                      # zeroed on the Dirichlet rows below; the caller's array stays as it is
        flags = _reduce_flag(reduce)
        ng = B.shape[1] // group_cols
        X = np.empty_like(B)
        its = np.zeros(ng, dtype=np.int32)
        errs = np.zeros(ng, dtype=np.float64)
        if masks is None:
            call('glx_cg_groups_masked', self._handle(), _ptr(B), _ptr(X), B.shape[1], int(group_cols), None, None, float(tol), int(max_iter), flags,
                 its.ctypes.data_as(C.POINTER(C.c_int)), errs.ctypes.data_as(_f64p))
            return X, its, errs
        if len(masks) != ng:
            raise GlxError('cg_groups: %d masks for %d systems' % (len(masks), ng))
        rows = [np.ascontiguousarray(m, dtype=np.int32).ravel() for m in masks]
        ptr = np.zeros(ng + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(r) for r in rows])
        allrows = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, np.int32), dtype=np.int32)
        for g, r in enumerate(rows):
            B[r, g * group_cols:(g + 1) * group_cols] = 0
        call('glx_cg_groups_masked', self._handle(), _ptr(B), _ptr(X), B.shape[1], int(group_cols), _ptr(allrows), _ptr(ptr), float(tol),
             int(max_iter), flags, its.ctypes.data_as(C.POINTER(C.c_int)), errs.ctypes.data_as(_f64p))
        return X, its, errs

    def cg_groups_rows(self, rows, vals, group_cols, masks, out_scale=None, tol=1e-10, max_iter=100000, reduce='exact'):
        """cg_groups for a right-hand side given by its nonzero rows (`rows` distinct, `vals` (len(rows), C); every other row
        zero -- and zero on the Dirichlet rows, which the caller guarantees), the result optionally scaled row by row on the
        device (glx_cg_groups_rows).  Returns (X, iterations per group, err per group); X is page-locked memory."""
        rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        vals = np.ascontiguousarray(vals, dtype=self.dtype)
        Cc = vals.shape[1]
        ng = Cc // group_cols
        if len(masks) != ng:
            raise GlxError('cg_groups_rows: %d masks for %d systems' % (len(masks), ng))
        mrows = [np.ascontiguousarray(m, dtype=np.int32).ravel() for m in masks]
        ptr = np.zeros(ng + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(r) for r in mrows])
        allrows = np.ascontiguousarray(np.concatenate(mrows) if mrows else np.zeros(0, np.int32), dtype=np.int32)
        scale = None if out_scale is None else _dense(out_scale, np.float64, (self.shape[0],), 'out_scale')
        X = pinned_empty((self.shape[0], Cc), self.dtype)
        its = np.zeros(ng, dtype=np.int32)
        errs = np.zeros(ng, dtype=np.float64)
        call('glx_cg_groups_rows', self._handle(), len(rows), _ptr(rows), _ptr(vals), _ptr(scale), _ptr(X), Cc, int(group_cols), _ptr(allrows),
             _ptr(ptr), float(tol), int(max_iter), _reduce_flag(reduce), its.ctypes.data_as(C.POINTER(C.c_int)), errs.ctypes.data_as(_f64p))
        return X, its, errs

    def last_block_stats(self):
        """(plain, by record, row by row) block counts of the last reference-order solve's reduction chains; (-1, -1, -1): chain form.
        `last_block_forms()`: which kinds of reduction ended the solve in block form (bit 0: p.Ap, bit 1: r.r)."""
        return self._block_stats()[:3]

    def last_block_forms(self):
        return self._block_stats()[3]

    def _block_stats(self):
        out = (C.c_int * 4)()
        call('glx_cg_last_block_stats', self._handle(), out)
        return tuple(out)

    def last_stop_margin(self):
        """How close the stop decisions of the last tolerance-mode solve on this operator came to going the other way (relative to
        tol; inf: no such solve)."""
        m = C.c_double(0)
        call('glx_cg_last_stop_margin', self._handle(), C.byref(m))
        return m.value


def host_fingerprint(arrays):
    """128-bit content fingerprint of a list of contiguous numpy arrays (glx_host_fingerprint: threaded, in the library), or
    None when the library is not there."""
    lib = load(required=False)
    if lib is None:
        return None
    out = (C.c_uint64 * 2)()
    acc = 0
    for a in arrays:
        call('glx_host_fingerprint', _ptr(a), a.nbytes, acc & 0xffffffffffffffff, out)
        acc = out[0] ^ ((out[1] * 0x9e3779b97f4a7c15) & 0xffffffffffffffff)
    return (int(out[0]), int(out[1]))


def _reduce_flag(reduce):
    if reduce == 'exact':
        if CG_EXACT_FORM not in (None, 'blocks', 'chain'):
            raise GlxError("CG_EXACT_FORM must be None, 'blocks' or 'chain', got %r" % (CG_EXACT_FORM,))
        return {None: 0, 'blocks': GLX_CG_BLOCKS, 'chain': GLX_CG_CHAIN}[CG_EXACT_FORM] | (GLX_CG_EAGER if CG_EXACT_EAGER else 0)
    if reduce == 'tree':
        return GLX_CG_TREE
    raise GlxError("reduce must be 'exact' (reference-order reductions) or 'tree' (tolerance mode), got %r" % (reduce,))


class Sweep(_Handle):
    """Prepared Poisson / heat sweep (glx_sweep): device-resident state, repeated runs."""

    _destroy = 'glx_sweep_destroy'

    def __init__(self, graph, Cc, min_iter=50, max_iter=1000, use_hipgraph=True):
        self.graph = graph
        self.C = Cc
        self.generation = 0
        self._open('glx_sweep_create', graph._handle(), Cc, min_iter, max_iter, 1 if use_hipgraph else 0)

    def set_problem(self, Db, w0, deg, vinf):
        n = self.graph.shape[0]
        Db = _dense(Db, self.graph.dtype, (n, self.C), 'Db')
        call('glx_sweep_set_problem', self._handle(), _ptr(Db), _ptr(_dense(w0, np.float64, (n,))), _ptr(_dense(deg, np.float64, (n,))),
             _ptr(_dense(vinf, np.float64, (n,))))

    def set_vectors(self, deg, vinf):
        """The graph's own vectors of the stop test (ssl.py:642-643), uploaded once per prepared sweep."""
        n = self.graph.shape[0]
        call('glx_sweep_set_vectors', self._handle(), _ptr(_dense(deg, np.float64, (n,))), _ptr(_dense(vinf, np.float64, (n,))))

    def set_problem_rows(self, rows, Db_rows, w0_rows, err0):
        """A new training set: the labelled rows, their rows of Db = D^-1 b and of w0 = v0/deg, and
        err0 = max|v0 - vinf| (ssl.py:620-622, 636, 639-641, 667)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        m = len(rows)
        Db_rows = _dense(Db_rows, self.graph.dtype, (m, self.C), 'Db_rows')
        w0_rows = _dense(w0_rows, np.float64, (m,), 'w0_rows')
        call('glx_sweep_set_problem_rows', self._handle(), m, _ptr(rows), _ptr(Db_rows), _ptr(w0_rows), float(err0))

    def run(self):
        T = C.c_int(0)
        ms = C.c_float(0)
        call('glx_sweep_run', self._handle(), C.byref(T), C.byref(ms))
        self.generation += 1
        return T.value, ms.value

    def stop_values(self):
        """(first, values): the stop values max|v_t - v_inf| the last run() compared with 1/n, t = first, first+1, ..."""
        first, count = C.c_int(0), C.c_int(0)
        call('glx_sweep_stop_values', self._handle(), 0, None, C.byref(first), C.byref(count))
        vals = np.empty(count.value, dtype=np.float64)
        call('glx_sweep_stop_values', self._handle(), len(vals), _ptr(vals), C.byref(first), C.byref(count))
        return first.value, vals

    def set_state(self, u0, Db=None):
        n = self.graph.shape[0]
        u0 = None if u0 is None else _dense(u0, self.graph.dtype, (n, self.C), 'u0')
        Db = None if Db is None else _dense(Db, self.graph.dtype, (n, self.C), 'Db')
        call('glx_sweep_set_state', self._handle(), _ptr(u0), _ptr(Db))
        self.generation += 1

    def set_state_labels(self, labels, rows, Db_rows):
        """u = onehot(labels), bias = its m nonzero rows (distinct `rows`): n labels and m rows go up instead of two dense arrays."""
        n = self.graph.shape[0]
        labels = _dense(labels, np.int64, (n,), 'labels')
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        Db_rows = _dense(Db_rows, self.graph.dtype, (len(rows), self.C), 'Db_rows')
        call('glx_sweep_set_state_labels', self._handle(), _ptr(labels), len(rows), _ptr(rows), _ptr(Db_rows))
        self.generation += 1

    def iterate(self, iters):
        call('glx_sweep_iterate', self._handle(), int(iters))
        self.generation += 1

    def fetch(self):
        out = pinned_empty((self.graph.shape[0], self.C), self.graph.dtype)
        call('glx_sweep_fetch', self._handle(), _ptr(out))
        return out

    def project(self, priors=None, weights=None, max_steps=0, similarity=True, to_onehot=False, want_labels=True, then_iterate=0):
        """ssl.predict / ssl.volume_label_projection on the device-resident state; with to_onehot the
        state becomes onehot(labels), and then_iterate sweeps are enqueued behind it at once (not awaited).
        Returns (labels int64 or None, weights, err, steps)."""
        n = self.graph.shape[0]
        w = np.ones(self.C) if weights is None else np.array(weights, dtype=np.float64).reshape(self.C).copy()
        pri = np.zeros(self.C) if priors is None else _dense(priors, np.float64, (self.C,), 'priors')
        labels = pinned_empty((n,), np.int64) if want_labels else None
        err = C.c_double(0)
        steps = C.c_int(0)
        call('glx_sweep_project_iterate', self._handle(), _ptr(pri), _ptr(w), _ptr(labels) if want_labels else None, C.byref(err), C.byref(steps),
             int(max_steps), 1 if similarity else 0, 1 if to_onehot else 0, int(then_iterate))
        if to_onehot or then_iterate:
            self.generation += 1
        return labels, w, err.value, steps.value

    def launches(self):
        n = C.c_int64(0)
        call('glx_sweep_launches', self._handle(), C.byref(n))
        return n.value


class SweepGroups(_Handle):
    """Several training sets as column groups of ONE prepared Poisson sweep (glx_sweep_groups): trial b owns columns
    b C .. b C + C - 1, its own stop value and its own stop test; every trial's iterate and T are those of its own fit."""

    _destroy = 'glx_sweep_groups_destroy'

    def __init__(self, graph, Cc, B, min_iter=50, max_iter=1000):
        self.graph = graph
        self.C = Cc
        self.B = B
        self.generation = 0
        self._open('glx_sweep_groups_create', graph._handle(), Cc, B, min_iter, max_iter)

    def set_vectors(self, deg, vinf):
        n = self.graph.shape[0]
        call('glx_sweep_groups_set_vectors', self._handle(), _ptr(_dense(deg, np.float64, (n,))), _ptr(_dense(vinf, np.float64, (n,))))

    def set_problem_rows(self, b, rows, Db_rows, w0_rows, err0):
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        m = len(rows)
        Db_rows = _dense(Db_rows, self.graph.dtype, (m, self.C), 'Db_rows')
        w0_rows = _dense(w0_rows, np.float64, (m,), 'w0_rows')
        call('glx_sweep_groups_set_problem_rows', self._handle(), int(b), m, _ptr(rows), _ptr(Db_rows), _ptr(w0_rows), float(err0))

    def run(self, used=None):
        """Returns (T per group in use, device ms)."""
        used = self.B if used is None else int(used)
        T = (C.c_int * self.B)()
        ms = C.c_float(0)
        call('glx_sweep_groups_run', self._handle(), used, T, C.byref(ms))
        self.generation += 1
        return [int(T[b]) for b in range(used)], ms.value

    def stop_values(self, b):
        first, count = C.c_int(0), C.c_int(0)
        call('glx_sweep_groups_stop_values', self._handle(), int(b), 0, None, C.byref(first), C.byref(count))
        vals = np.empty(count.value, dtype=np.float64)
        call('glx_sweep_groups_stop_values', self._handle(), int(b), len(vals), _ptr(vals), C.byref(first), C.byref(count))
        return first.value, vals

    def fetch(self, b):
        out = pinned_empty((self.graph.shape[0], self.C), self.graph.dtype)
        call('glx_sweep_groups_fetch', self._handle(), int(b), _ptr(out))
        return out

    def project(self, b, priors=None, weights=None, max_steps=0, similarity=True, want_labels=True):
        n = self.graph.shape[0]
        w = np.ones(self.C) if weights is None else np.array(weights, dtype=np.float64).reshape(self.C).copy()
        pri = np.zeros(self.C) if priors is None else _dense(priors, np.float64, (self.C,), 'priors')
        labels = pinned_empty((n,), np.int64) if want_labels else None
        err = C.c_double(0)
        steps = C.c_int(0)
        call('glx_sweep_groups_project', self._handle(), int(b), _ptr(pri), _ptr(w), _ptr(labels) if want_labels else None, C.byref(err),
             C.byref(steps), int(max_steps), 1 if similarity else 0)
        return labels, w, err.value, steps.value

    def launches(self):
        n = C.c_int64(0)
        call('glx_sweep_groups_launches', self._handle(), C.byref(n))
        return n.value

    def view(self, b):
        return GroupView(self, b)


class GroupView:
    """Group b of a SweepGroups with the face of a Sweep (C, fetch, project, generation, _h): what ssl._DeviceState needs to leave a
    trial's result on the device until somebody looks at it."""

    def __init__(self, groups, b):
        self.groups, self.b, self.C = groups, int(b), groups.C

    @property
    def _h(self):
        return self.groups._h

    @property
    def generation(self):
        return self.groups.generation

    def fetch(self):
        return self.groups.fetch(self.b)

    def project(self, priors=None, weights=None, max_steps=0, similarity=True, to_onehot=False, want_labels=True, then_iterate=0):
        if to_onehot or then_iterate:
            raise GlxError('a stacked trial has no heat loop of its own')
        return self.groups.project(self.b, priors, weights, max_steps=max_steps, similarity=similarity, want_labels=want_labels)


class Comm(_Handle):
    """One rank's libglx-owned RCCL communicator (glx_comm).  `uid`: the 128 bytes of Comm.unique_id() made on rank 0
    and shipped to every rank; uid=None with nranks == 1 gives a transport-free single rank."""

    _destroy = 'glx_dist_destroy'
    _abandon_at_exit = True

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        call('glx_dist_unique_id', buf)
        return buf.raw

    def __init__(self, nranks=1, rank=0, uid=None, device=None):
        self.nranks, self.rank, self.device = int(nranks), int(rank), _dev(device)
        idbuf = None if uid is None else C.create_string_buffer(bytes(uid), 128)
        self._open('glx_dist_init_rank', self.nranks, self.rank, idbuf, self.device)

    def info(self):
        info = (C.c_int32 * 4)()
        call('glx_dist_comm_info', self._handle(), info)
        return dict(rank=int(info[0]), nranks=int(info[1]), device=int(info[2]), rccl=bool(info[3]))

    def has_transport(self):
        return self.info()['rccl']


# glx_dist_sweep_create's form flags (include/glx.h): what the library picks by itself, and the forms tests force
DIST_FORMS = {'auto': 0, 'split': 2, 'split_pack': 2 | 8, 'split_inline': 2 | 16, 'fused': 4, 'selftest': 128, 'eager': 64, 'captured': 32}
DIST_GATHER = 256        # GLX_DIST_FORM_GATHER: the exchange is one in-place all-gather of the ranks' blocks (dist.GatherPlan)


class DistSweep(_Handle):
    """One rank's share of the vertex-partitioned Poisson sweep (glx_dist_sweep): local operator (boundary rows first,
    columns [owned | halo]), exchange lists, device state; every sweep and every collective is enqueued by libglx."""

    _destroy = 'glx_dist_sweep_destroy'
    _abandon_at_exit = True

    def __init__(self, comm, P_local, n_boundary, send_counts, send_idx, recv_counts, n_global, Cc, dtype=np.float64,
                 force_exchange=False, use_hipgraph=True, form='auto', gather_cap=None):
        """gather_cap (dist.GatherPlan): the all-gather form -- P_local's columns are numbered owner * cap + (row within the owner's
        block), shape (n_own, world * cap); the exchange lists are not used."""
        from scipy import sparse
        A = sparse.csr_matrix(P_local)
        self.comm = comm
        self.n_own, n_loc = A.shape
        self.gather_cap = None if gather_cap is None else int(gather_cap)
        self.n_halo = n_loc - (self.n_own if gather_cap is None else self.gather_cap)
        self.C = int(Cc)
        self.dtype = np.dtype(dtype)
        self.lay = record_layout(Cc, dtype, True)
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        rcnt = np.ascontiguousarray(recv_counts, dtype=np.int64)
        si = np.ascontiguousarray(send_idx, dtype=np.int32)
        self.n_send = int(sc.sum()) if gather_cap is None else self.gather_cap
        flags = (1 if use_hipgraph else 0) | DIST_FORMS[form] | (DIST_GATHER if gather_cap is not None else 0)
        self._open('glx_dist_sweep_create', comm._handle(), self.n_own, self.n_halo, int(n_boundary), _ptr(rowptr), _ptr(col), _ptr(val),
                   _dt(self.dtype), self.C, _ptr(sc), _ptr(si), _ptr(rcnt), int(n_global), 1 if force_exchange else 0, flags)

    def set_problem(self, Db_own, w0_own, deg_own, vinf_own):
        n = self.n_own
        Db = None if Db_own is None else _dense(Db_own, self.dtype, (n, self.C), 'Db_own')
        call('glx_dist_sweep_set_problem', self._handle(), _ptr(Db), _ptr(_dense(w0_own, np.float64, (n,))), _ptr(_dense(deg_own, np.float64, (n,))),
             _ptr(_dense(vinf_own, np.float64, (n,))))

    def run(self, min_iter=50, max_iter=1000, check_every=8, err0=0.0):
        T = C.c_int(0)
        ms = C.c_float(0)
        call('glx_poisson_sweep_dist', self._handle(), int(min_iter), int(max_iter), int(check_every), float(err0), C.byref(T), C.byref(ms))
        return T.value, ms.value

    def fetch(self):
        out = np.empty((self.n_own, self.C), dtype=self.dtype)
        call('glx_dist_sweep_fetch', self._handle(), _ptr(out))
        return out

    def stats(self):
        out = (C.c_int64 * 4)()
        call('glx_dist_sweep_stats', self._handle(), out)
        return dict(sweeps=out[0], exchanges=out[1], graphs=out[2], exchanging=bool(out[3]))

    def info(self):
        """What the object decided (glx_dist_sweep_info): captured / eager exchanging sweeps, the self-test's verdict, ..."""
        out = (C.c_int64 * 8)()
        call('glx_dist_sweep_info', self._handle(), out)
        cap = {1: 'captured', 0: 'eager', -1: 'undecided'}[int(out[1])]
        return dict(exchanging=bool(out[0]), exchange=cap if out[0] else 'none', selftest={0: 'not run', 1: 'passed', 2: 'failed'}[int(out[2])],
                    overlap=bool(out[3]), fused=bool(out[4]), scatter=bool(out[5]), send_records=int(out[6]), halo_records=int(out[7]))

    def time_parts(self, reps=50):
        """Microseconds of the rank-local pieces of one sweep, each timed alone (glx_dist_sweep_time_parts)."""
        out = (C.c_float * 4)()
        call('glx_dist_sweep_time_parts', self._handle(), int(reps), out)
        return dict(boundary_us=float(out[0]), interior_us=float(out[1]), pack_us=float(out[2]), both_us=float(out[3]))

    # stepwise form (transport left to the caller)
    def begin(self):
        call('glx_dist_sweep_begin', self._handle())

    def boundary(self, want_err):
        call('glx_dist_sweep_boundary', self._handle(), 1 if want_err else 0)

    def get_send(self):
        out = np.empty((self.n_send, self.lay['ld']), dtype=self.dtype)
        call('glx_dist_sweep_get_send', self._handle(), _ptr(out))
        return out

    def put_halo(self, rec, next_iterate):
        rec = _dense(rec, self.dtype, (self.n_halo, self.lay['ld']), 'halo records')
        call('glx_dist_sweep_put_halo', self._handle(), _ptr(rec), 1 if next_iterate else 0)

    def interior(self, want_err):
        e = C.c_double(0)
        call('glx_dist_sweep_interior', self._handle(), 1 if want_err else 0, C.byref(e))
        return e.value if want_err else None


def nearest_dist(X, idx, device=None):
    """Distance from every row of X to the nearest of its rows `idx` (glx_nearest_dist: cKDTree(X[idx]).query(X)[0], bit for bit).
    GlxError for an empty `idx`, an index outside [0, n), more than 6144 features, and for a NaN or an infinity anywhere in X (the
    reference's cKDTree raises on non-finite data; weightmatrix.epsilon_ball refuses it too)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise GlxError('nearest_dist: X must be (n, d)')
    idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), dtype=np.int64)
    out = np.empty(X.shape[0], dtype=np.float64)
    call('glx_nearest_dist', _ptr(X), X.shape[0], X.shape[1], _ptr(idx), len(idx), _ptr(out), _dev(device))
    return out


def record_layout(Cc, dtype=np.float64, has_w=True):
    """Vertex-record layout of the dense operands (pure host call, no GPU needed)."""
    out = (C.c_int32 * 6)()
    call('glx_record_layout', int(Cc), _dt(dtype), 1 if has_w else 0, out)
    return dict(ld=out[0], woff=out[1], rec_bytes=out[2], G=out[3], nvec=out[4], esize=out[5])


def argmax_project(prob, priors=None, weights=None, max_steps=0, similarity=True, device=None):
    """ssl.predict / ssl.volume_label_projection on device.
    Returns (labels int64, weights, err, steps)."""
    prob = np.asarray(prob)
    # a float32 prob (use_cuda=True) is normalised in float32 like numpy would (ssl.py:256-257)
    prob = np.ascontiguousarray(prob, dtype=np.float32 if prob.dtype == np.float32 else np.float64)
    n, Cc = prob.shape
    w = np.ones(Cc) if weights is None else np.array(weights, dtype=np.float64).reshape(Cc).copy()
    pri = np.zeros(Cc) if priors is None else _dense(priors, np.float64, (Cc,), 'priors')
    labels = np.empty(n, dtype=np.int64)
    err = C.c_double(0)
    steps = C.c_int(0)
    call('glx_argmax_project_t', _ptr(prob), _dt(prob.dtype), n, Cc, _ptr(pri), _ptr(w), _ptr(labels), C.byref(err), C.byref(steps), int(max_steps),
         1 if similarity else 0, _dev(device))
    return labels, w, err.value, steps.value


def lp_iterate(uu, ul, nbr, row, W, ind, val, p, T, tol, device=None):
    """lp_iterate of the reference's C extension on the GPU (in place on uu, ul); returns the stopping iteration."""
    for a, dt in ((uu, np.float64), (ul, np.float64), (nbr, np.int32), (row, np.int32), (W, np.float64), (ind, np.int32), (val, np.float64)):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags['C_CONTIGUOUS']):
            raise GlxError('lp_iterate: arrays must be C-contiguous with the dtypes of the reference binding')
    it = C.c_int64(0)
    call('glx_lp_iterate', _ptr(uu), _ptr(ul), _ptr(nbr), _ptr(row), _ptr(W), _ptr(ind), _ptr(val), float(p), int(T), float(tol), len(uu), len(W),
         len(ind), C.byref(it), _dev(device))
    return it.value


def lp_iterate_batch(n, nbr, row, W, ind, val, p, T, tol, device=None):
    """B problems of `lp_iterate` that share the boundary vertices `ind`, one per column of `val` (m, B), in one device call
    (glx_lp_iterate_batch, csrc/plaplace.hip): column b starts from uu = max(val[:, b]), ul = min(val[:, b]) off the boundary.  Returns
    (uu (n, B), ul (n, B), stopping iteration per column (B,) int64); every column equals its own `lp_iterate` call bit for bit."""
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    row = np.ascontiguousarray(row, dtype=np.int32)
    W = np.ascontiguousarray(W, dtype=np.float64)
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    if val.ndim != 2 or val.shape[0] != len(ind) or nbr.ndim != 1 or len(nbr) != len(row) or len(nbr) != len(W) or ind.ndim != 1:
        raise GlxError('lp_iterate_batch: inconsistent array shapes')
    n, B, T = int(n), int(val.shape[1]), int(T)
    if n < 1 or B < 1 or T < 0:
        raise GlxError('lp_iterate_batch: bad sizes (n=%d B=%d T=%d)' % (n, B, T))
    uu = np.empty((n, B), dtype=np.float64)
    ul = np.empty((n, B), dtype=np.float64)
    iters = np.zeros(B, dtype=np.int64)
    call('glx_lp_iterate_batch', n, len(nbr), _ptr(nbr), _ptr(row), _ptr(W), B, len(ind), _ptr(ind), _ptr(val), float(p), T, float(tol), _ptr(uu),
         _ptr(ul), _ptr(iters), _dev(device))
    return uu, ul, iters


GLX_SSSP_PLAIN, GLX_SSSP_HOPF_LAX = 0, 1


SSSP_FULL_SWEEPS = False        # True: every round looks at every value (no out-edge lists are handed over); same results, for measurement
sssp_last_ms = None             # host milliseconds of the last call: uploads, distance rounds, closest-point rounds, downloads


def sssp(in_ptr, in_idx, in_cost, src_ptr, src_idx, src_val, max_dist=np.inf, hopf_lax=False, return_cp=False, device=None,
         out_ptr=None, out_idx=None):
    """Shortest-path distances of B = len(src_ptr) - 1 problems on one graph given by its in-edge lists (glx_sssp, csrc/sssp.hip):
    returns (dist (n, B) float64, cp (n, B) int32 or None, (distance rounds, closest-point rounds)).  out_ptr / out_idx: the same
    edges by the vertex they leave (rounds then only look at values whose in-neighbours moved)."""
    global sssp_last_ms
    if out_ptr is None or SSSP_FULL_SWEEPS:
        out_ptr = out_idx = None
    else:
        out_ptr = np.ascontiguousarray(out_ptr, dtype=np.int64)
        out_idx = np.ascontiguousarray(out_idx, dtype=np.int32)
        if len(out_ptr) != len(in_ptr) or len(out_idx) != len(in_idx):
            raise GlxError('sssp: the out-edge lists do not match the in-edge lists')
    in_ptr = np.ascontiguousarray(in_ptr, dtype=np.int64)
    in_idx = np.ascontiguousarray(in_idx, dtype=np.int32)
    in_cost = np.ascontiguousarray(in_cost, dtype=np.float64)
    src_ptr = np.ascontiguousarray(src_ptr, dtype=np.int64)
    src_idx = np.ascontiguousarray(src_idx, dtype=np.int32)
    src_val = np.ascontiguousarray(src_val, dtype=np.float64)
    n, B = len(in_ptr) - 1, len(src_ptr) - 1
    if n < 1 or B < 1 or len(in_idx) != len(in_cost) or len(src_idx) != len(src_val):
        raise GlxError('sssp: inconsistent array lengths')
    dist = np.empty((n, B), dtype=np.float64)
    cp = np.empty((n, B), dtype=np.int32) if return_cp else None
    rounds = (C.c_int64 * 2)(0, 0)
    ms = (C.c_double * 4)(0, 0, 0, 0)
    call('glx_sssp', n, len(in_idx), _ptr(in_ptr), _ptr(in_idx), _ptr(in_cost), _ptr(out_ptr), _ptr(out_idx), B, _ptr(src_ptr), _ptr(src_idx),
         _ptr(src_val), float(max_dist), GLX_SSSP_HOPF_LAX if hopf_lax else GLX_SSSP_PLAIN, _ptr(dist), _ptr(cp), rounds, ms, _dev(device))
    sssp_last_ms = tuple(ms)
    return dist, cp, (int(rounds[0]), int(rounds[1]))


components_last_ms = None       # host milliseconds of the last call: uploads, checks, kernels, downloads


def int32_index_array(a, name):
    """`a` as a contiguous int32 array; ValueError if a value does not fit (a cast would wrap it into range)"""
    a = np.asarray(a)
    if a.dtype != np.int32:
        if a.dtype.kind not in 'iu':
            raise ValueError('%s: an integer array is expected, not %s' % (name, a.dtype))
        if a.size and (int(a.min()) < -(1 << 31) or int(a.max()) > (1 << 31) - 1):
            raise ValueError('%s holds values that are not int32-representable' % name)
    return np.ascontiguousarray(a, dtype=np.int32)


def components(indptr, indices, n, device=None):
    """Connected components of the pattern of an n x n CSR matrix given by its raw index arrays (glx_components, csrc/cc.hip): every
    stored entry joins its row and its column, whatever its value.  Returns (ncomp, labels int32 (n,)) with scipy's numbering --
    components in the order of their smallest vertex.  Malformed arrays are refused with GlxError before a kernel follows an index."""
    global components_last_ms
    indptr = int32_index_array(indptr, 'indptr')
    indices = int32_index_array(indices, 'indices')
    n = int(n)
    if n < 1 or indptr.ndim != 1 or indices.ndim != 1 or len(indptr) != n + 1:
        raise GlxError('components: indptr has %s entries for n = %d' % (indptr.shape, n))
    labels = np.empty(n, dtype=np.int32)
    ncomp = C.c_int64(0)
    ms = (C.c_double * 4)(0, 0, 0, 0)
    call('glx_components', n, len(indices), _ptr(indptr), _ptr(indices), _ptr(labels), C.byref(ncomp), ms, _dev(device))
    components_last_ms = tuple(ms)
    return int(ncomp.value), labels


def components_set_wave_row(min_entries=0):
    """plan override of the calling thread for measurements: rows of at least `min_entries` stored entries take a wavefront (0: the library's)"""
    call('glx_components_set_wave_row', int(min_entries))


def components_plan():
    """(threshold in effect, the library's own, vertices per scan tile, rows that took a wavefront in this thread's last call)"""
    out = (C.c_int64 * 4)()
    call('glx_components_plan', out)
    return tuple(int(v) for v in out)


BSTAT_SECOND_ORDER, BSTAT_CUTOFF = 1, 2          # flags of glx_boundary_stat (include/glx_experimental.h)
# of the last call: launches, rows of the short class, rows on a wavefront, rows of the largest length, host milliseconds of the
# checks, uploads, kernels, downloads
boundary_stat_last = None


def boundary_stat(X, indptr, indices, second_order=True, cutoff=True, J=None, device=None):
    """The boundary statistic over a canonical CSR pattern with unit weights (glx_boundary_stat, csrc/bstat.hip).  X (n, d) float64;
    J (n, k) the neighbour lists of the kNN mode, None: the radius mode.  Returns (T (n,), nu (n, d)) float64.  Malformed arrays, an
    empty row and a normal of norm zero are refused with GlxError."""
    global boundary_stat_last
    X = _dense(X, np.float64, name='X')
    if X.ndim != 2:
        raise GlxError('boundary_stat: X must be (n, d), got shape %s' % (X.shape,))
    n, d = X.shape
    indptr = int32_index_array(indptr, 'indptr')
    indices = int32_index_array(indices, 'indices')
    if indptr.ndim != 1 or indices.ndim != 1 or len(indptr) != n + 1:
        raise GlxError('boundary_stat: indptr has %s entries for n = %d' % (indptr.shape, n))
    k = 0
    if J is not None:
        J = int32_index_array(J, 'J')
        if J.ndim != 2 or J.shape[0] != n or J.shape[1] < 1:
            raise GlxError('boundary_stat: J has shape %s for n = %d' % (J.shape, n))
        k = J.shape[1]
    T, nu = np.empty(n), np.empty((n, d))
    stats = (C.c_double * 8)()
    flags = (BSTAT_SECOND_ORDER if second_order else 0) | (BSTAT_CUTOFF if cutoff else 0)
    call('glx_boundary_stat', n, d, _ptr(X), len(indices), _ptr(indptr), _ptr(indices), k, _ptr(J), flags, _ptr(T), _ptr(nu), stats,
         _dev(device))
    boundary_stat_last = tuple(stats)
    return T, nu


def boundary_stat_set_wave_row(min_members=0):
    """plan override of the calling thread for measurements: rows of at least `min_members` members take a wavefront (0: the library's)"""
    call('glx_boundary_stat_set_wave_row', int(min_members))


peikonal_last_ms = None         # host milliseconds of the last call: uploads, rounds, download


def peikonal(row_ptr, nbr, W, f, bdy_ptr, bdy_idx, bdy_val, p, num_bisection_it, u0, device=None, max_rounds=0):
    """The p-eikonal equation for B = len(bdy_ptr) - 1 boundary sets on one graph (glx_peikonal, csrc/peik.hip): the stored entries
    sorted by vertex (row_ptr (n + 1), nbr, W), f (n), the boundary lists and their values, u0 (n) for vertices no boundary reaches.
    Returns (u (n, B) float64, rounds).  max_rounds: 0, or a cap below the library's own (peik_round_cap of csrc/peik_plan.h; a test hook)."""
    global peikonal_last_ms
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    W = np.ascontiguousarray(W, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    u0 = np.ascontiguousarray(u0, dtype=np.float64)
    bdy_ptr = np.ascontiguousarray(bdy_ptr, dtype=np.int64)
    bdy_idx = np.ascontiguousarray(bdy_idx, dtype=np.int32)
    bdy_val = np.ascontiguousarray(bdy_val, dtype=np.float64)
    n, B = len(row_ptr) - 1, len(bdy_ptr) - 1
    if (n < 1 or B < 1 or nbr.ndim != 1 or len(nbr) != len(W) or f.shape != (n,) or u0.shape != (n,) or bdy_idx.ndim != 1
            or len(bdy_idx) != len(bdy_val) or len(bdy_idx) != bdy_ptr[-1]):
        raise GlxError('peikonal: inconsistent array shapes')
    u = np.empty((n, B), dtype=np.float64)
    rounds = C.c_int64(0)
    ms = (C.c_double * 3)(0, 0, 0)
    call('glx_peikonal', n, len(nbr), _ptr(row_ptr), _ptr(nbr), _ptr(W), _ptr(f), B, _ptr(bdy_ptr), _ptr(bdy_idx), _ptr(bdy_val), float(p),
         int(num_bisection_it), _ptr(u0), int(max_rounds), _ptr(u), C.byref(rounds), ms, _dev(device))
    peikonal_last_ms = tuple(ms)
    return u, int(rounds.value)


def lip_iterate(n, nbr, row, W, ind, val, weighted, alpha, beta, T, tol, device=None, want_errors=False, small_level=-1):
    """In-order Gauss-Seidel sweeps of the reference's lip_iterate on the GPU (glx_lip_iterate, csrc/lip.hip): n vertices, the entry
    arrays as the reference hands them over (nbr = graph.J, row = graph.I, W = graph.V), the shared boundary vertices `ind` and their
    values `val` (m, B).  Returns (u (n, B) float64, sweeps done per column (B,) int64, plan = (levels, launches per sweep, launches
    enqueued in all), errors (T, B) or None: rows a column did not run hold NaN).  small_level: a plan override for measurements --
    levels of at most that many vertices ride in merged launches (0: none; -1: the library's constant); the result does not depend on it."""
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    row = np.ascontiguousarray(row, dtype=np.int32)
    W = np.ascontiguousarray(W, dtype=np.float64)
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    if val.ndim != 2 or val.shape[0] != len(ind) or nbr.ndim != 1 or len(nbr) != len(row) or len(nbr) != len(W) or ind.ndim != 1:
        raise GlxError('lip_iterate: inconsistent array shapes')
    n, B, T = int(n), int(val.shape[1]), int(T)
    if n < 1 or B < 1 or T < 0:
        raise GlxError('lip_iterate: bad sizes (n=%d B=%d T=%d)' % (n, B, T))
    u = np.empty((n, B), dtype=np.float64)
    iters = np.zeros(B, dtype=np.int64)
    plan = (C.c_int64 * 3)(0, 0, 0)
    errs = np.full((T, B), np.nan) if want_errors else None
    call('glx_lip_iterate', n, len(nbr), _ptr(nbr), _ptr(row), _ptr(W), B, len(ind), _ptr(ind), _ptr(val), 1 if weighted else 0, float(alpha),
         float(beta), T, float(tol), _ptr(u), _ptr(iters), plan, _ptr(errs), int(small_level), _dev(device))
    return u, iters, (int(plan[0]), int(plan[1]), int(plan[2])), errs


def _csr_operands(row_ptr, col, entries, ind=None, val=None):
    """The arrays of a one-call solver as the library takes them: (ok, n, row_ptr int64, col int32, the per-entry arrays float64, ind
    int32, val float64), all contiguous.  ok: row_ptr is (n + 1) with n >= 1, col (M), every per-entry array (M), and -- where given --
    ind (m) and val (m, k) with k >= 1.  The caller adds its own conditions and raises its own GlxError."""
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    entries = [np.ascontiguousarray(a, dtype=np.float64) for a in entries]
    n = len(row_ptr) - 1
    ok = row_ptr.ndim == 1 and n >= 1 and col.ndim == 1 and all(a.shape == col.shape for a in entries)
    if ind is not None:
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        ok = ok and ind.ndim == 1 and val.ndim == 2 and val.shape[0] == len(ind) and val.shape[1] >= 1
    return (ok, n, row_ptr, col, *entries, ind, val)


def slp_iterate(row_ptr, col, W, lam, gamma, ind, val, T, device=None, want_history=False):
    """T iterations of sparse label propagation on the GPU (glx_slp_iterate, csrc/slp.hip; the contract is DESIGN.md 4.9): W as
    canonical CSR arrays (row_ptr, col, W), lam per entry, gamma per vertex, the labelled vertices `ind` and the rows `val` (m, C) they are
    set to.  Returns (u (n, C) float64, the iterates (T, n, C) or None, plan = (launches per iteration, launches enqueued, column tile))."""
    ok, n, row_ptr, col, W, lam, ind, val = _csr_operands(row_ptr, col, (W, lam), ind, val)
    gamma, T = np.ascontiguousarray(gamma, dtype=np.float64), int(T)
    if not (ok and gamma.shape == (n,) and T >= 0):
        raise GlxError('slp_iterate: inconsistent array shapes or sizes')
    Cc = int(val.shape[1])
    u = np.empty((n, Cc), dtype=np.float64)
    hist = np.empty((T, n, Cc), dtype=np.float64) if want_history else None
    plan = (C.c_int64 * 3)(0, 0, 0)
    call('glx_slp_iterate', n, len(col), _ptr(row_ptr), _ptr(col), _ptr(W), _ptr(lam), _ptr(gamma), Cc, len(ind), _ptr(ind), _ptr(val), T, _ptr(u),
         _ptr(hist) if (want_history and T > 0) else None, plan, _dev(device))
    return u, hist, (int(plan[0]), int(plan[1]), int(plan[2]))


def ck_solve(row_ptr, col, W, ind, val, e, power_it=100, alpha_frac=1.05, tol=1e-10, max_it=1 << 24, device=None, err_cap=0, on_iterate=None):
    """The centered-kernel learner's two loops in one device call (glx_ck_solve, csrc/ck.hip; the contract is DESIGN.md 4.11): W as
    canonical CSR arrays (row_ptr, col, W) without its diagonal, the training vertices `ind` with their start rows `val` (m, k), the
    power iteration's start vector e (n).  Returns (u (n, k) float64, l, T, err (err_cap values: err_q at [q - 1] for q <= T, NaN behind), plan = (kernels per
    iteration, launches enqueued, iterations per chunk, partial sums per column)).  on_iterate(q, u_q, err_q), if given, is called after
    every iteration with a view of the iterate that is valid during the call only; the solve then runs one iteration per chunk and
    downloads every iterate (slow).  GlxError when max_it iterations pass without a stop."""
    ok, n, row_ptr, col, W, ind, val = _csr_operands(row_ptr, col, (W,), ind, val)
    e = np.ascontiguousarray(e, dtype=np.float64).ravel()
    if not (ok and e.shape == (n,) and int(err_cap) >= 0):
        raise GlxError('ck_solve: inconsistent array shapes or sizes')
    k = int(val.shape[1])
    u = np.empty((n, k), dtype=np.float64)
    errs = np.full(int(err_cap), np.nan)
    l, T = C.c_double(0.0), C.c_int64(0)
    plan = (C.c_int64 * 4)(0, 0, 0, 0)
    raised = []
    cb = None
    if on_iterate is not None:
        def _each(q, ptr, err, _user):
            try:
                on_iterate(int(q), np.ctypeslib.as_array(ptr, shape=(n, k)), float(err))
                return 0
            except BaseException as exc:      # an exception cannot cross the C frames: end the call and raise it afterwards
                raised.append(exc)
                return 1
        cb = _CK_ITERATE_FN(_each)
    try:
        call('glx_ck_solve', n, len(col), _ptr(row_ptr), _ptr(col), _ptr(W), k, len(ind), _ptr(ind), _ptr(val), _ptr(e), int(power_it),
             float(alpha_frac), float(tol), int(max_it), _ptr(u), C.byref(l), C.byref(T), _ptr(errs) if err_cap else None, int(err_cap),
             C.cast(cb, _vp) if cb is not None else None, None, plan, _dev(device))
    except GlxError:
        if raised:
            raise raised[0]
        raise
    return u, float(l.value), int(T.value), errs, tuple(int(v) for v in plan)


_CK_ITERATE_FN = C.CFUNCTYPE(C.c_int, C.c_int64, C.POINTER(C.c_double), C.c_double, _vp)


def dlp_solve(row_ptr, col, P, ind, val, alpha=0.05, lam=0.1, T=2, device=None, want_history=False):
    """Dynamic label propagation in one device call and without the dense n x n array (glx_dlp_solve, csrc/dlp.hip; the contract is
    DESIGN.md 4.17): P as canonical CSR arrays (row_ptr, col, P), the training vertices `ind` with their rows `val` (m, k).  Returns
    (u_T (n, k) float64, hist (T, n, k) = u_1 .. u_T or None, plan = (launches enqueued, sparse passes, Gram passes, partial sums per
    Gram entry))."""
    ok, n, row_ptr, col, P, ind, val = _csr_operands(row_ptr, col, (P,), ind, val)
    T = int(T)
    if not ok:
        raise GlxError('dlp_solve: inconsistent array shapes or sizes')
    k = int(val.shape[1])
    u = np.empty((n, k), dtype=np.float64)
    hist = np.empty((T, n, k), dtype=np.float64) if (want_history and 1 <= T <= 64) else None
    plan = (C.c_int64 * 4)(0, 0, 0, 0)
    call('glx_dlp_solve', n, len(col), _ptr(row_ptr), _ptr(col), _ptr(P), k, len(ind), _ptr(ind), _ptr(val), float(alpha), float(lam), T, _ptr(u),
         _ptr(hist) if hist is not None else None, plan, _dev(device))
    return u, hist, tuple(int(v) for v in plan)


def mmbo_solve(X, vals, lab0, ind, lab, k, Ns=6, T=10, dt=0.15, mu=50, device=None):
    """The multiclass MBO learner's T * Ns diffusion steps and T projections in one device call (glx_mmbo_solve, csrc/mmbo.hip; the
    contract is DESIGN.md 4.13): the basis X (n, m) with vals (m) -- any finite arrays, the learner hands in eigenpairs --, the start
    labels lab0 (n) in [0, k), the training vertices `ind` with their labels `lab`.  Returns (labels (T, n) int32 after every outer
    iteration, the last row being the result; the last Z (k, m) float64; plan = (launches per step, rows per partial sum, partial
    sums, the caps on k * m, k and m, launches enqueued)).  GlxError (GLX_EUNSUPPORTED) above the caps, before anything is touched."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    vals = np.ascontiguousarray(vals, dtype=np.float64).ravel()
    lab0 = np.ascontiguousarray(lab0, dtype=np.int32).ravel()
    ind = np.ascontiguousarray(ind, dtype=np.int32).ravel()
    lab = np.ascontiguousarray(lab, dtype=np.int32).ravel()
    k, Ns, T = int(k), int(Ns), int(T)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or vals.shape != (X.shape[1],) or lab0.shape != (X.shape[0],) or ind.shape != lab.shape:
        raise GlxError('mmbo_solve: inconsistent array shapes or sizes')
    n, m = X.shape
    ok = 1 <= k and 1 <= T and T * n <= 1 << 31 and k * m <= 1 << 16          # (the call refuses; only the result arrays depend on it)
    hist = np.empty((T, n) if ok else (1, 1), dtype=np.int32)
    Z = np.empty((k, m) if ok else (1, 1), dtype=np.float64)
    plan = (C.c_int64 * 7)(0, 0, 0, 0, 0, 0, 0)
    call('glx_mmbo_solve', n, m, _ptr(X), _ptr(vals), _ptr(lab0), len(ind), _ptr(ind), _ptr(lab), k, Ns, T, float(dt), float(mu), _ptr(hist), _ptr(Z),
         plan, _dev(device))
    return hist, Z, tuple(int(v) for v in plan)


class Eig(_Handle):
    """The device half of the thick-restart Lanczos eigensolver (glx_eig_*, csrc/eig.hip; the contract is DESIGN.md 4.12): a
    symmetric matrix A as canonical CSR arrays (row_ptr, col, val) and a basis of m + 1 column-major Lanczos vectors that stays on
    the device.  The backend interface of graphlearning_amd._eig.thick_restart: set_column, orthonormalize, run, rotate,
    get_columns.  A context manager; close() releases the device memory.  GlxError on every refusal of the library."""

    _destroy = 'glx_eig_destroy'

    def __init__(self, row_ptr, col, val, m, device=None):
        ok, n, row_ptr, col, val, _, _ = _csr_operands(row_ptr, col, (val,))
        if not (ok and int(row_ptr[-1]) == len(col)):
            raise GlxError('Eig: inconsistent array shapes or sizes')
        self.n, self.m = n, int(m)
        self._open('glx_eig_create', n, _ptr(row_ptr), _ptr(col), _ptr(val), int(m), _dev(device))

    def set_column(self, j, x):
        x = _dense(np.asarray(x).ravel(), np.float64, (self.n,), 'column')
        call('glx_eig_set_column', self._handle(), int(j), _ptr(x))

    def orthonormalize(self, j):
        norm = C.c_double(0.0)
        call('glx_eig_orthonormalize', self._handle(), int(j), C.byref(norm))
        return float(norm.value)

    def run(self, j0, j1):
        count = max(int(j1) - int(j0), 1)
        alpha, beta = np.empty(count), np.empty(count)
        call('glx_eig_run', self._handle(), int(j0), int(j1), _ptr(alpha), _ptr(beta))
        return alpha, beta

    def rotate(self, Y, rows, keep):
        Y = _dense(Y, np.float64, (int(rows), int(keep)), 'Y')
        call('glx_eig_rotate', self._handle(), _ptr(Y), int(rows), int(keep))

    def get_columns(self, j0, j1):
        """(n, j1 - j0): the columns j0 .. j1 - 1 of the basis"""
        out = np.empty((max(int(j1) - int(j0), 1), self.n))
        call('glx_eig_get_columns', self._handle(), int(j0), int(j1), _ptr(out))
        return np.ascontiguousarray(out.T)


def host_group_by_label(labels, k):
    """(counts (k) int64, order (n) int32): the vertex ids sorted by label, ascending inside a label (glx_host_group_by_label, a
    counting sort on the host; no device is touched).  GlxError for a label outside [0, k)."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    counts = np.empty(int(k), dtype=np.int64)
    order = np.empty(len(labels), dtype=np.int32)
    call('glx_host_group_by_label', len(labels), _ptr(labels), int(k), _ptr(counts), _ptr(order))
    return counts, order


class _IncresOptions(C.Structure):
    _fields_ = [('chunk', C.c_int), ('margin', C.c_int), ('next', C.c_int)]


class incres_options:
    """Context manager: the schedule of the calling thread's INCRES grow loops (glx_incres_set_options) -- chunk: sweeps between two
    reads of the flags, every chunk alike; margin: the first chunk of a loop is the count of the loop before plus this; next: the
    length of a loop's second chunk, every further one twice as long (each 1 .. 64, None: the library decides).  Every schedule gives the same labels and counts; tests and
    measurements use this."""

    def __init__(self, chunk=None, margin=None, next=None):
        self.opt = _IncresOptions(int(chunk or 0), int(margin or 0), int(next or 0))

    def __enter__(self):
        call('glx_incres_set_options', C.byref(self.opt))
        return self

    def __exit__(self, *exc):
        load().glx_incres_set_options(None)
        return False


class Incres(_Handle):
    """The device half of clustering.incres (glx_incres_*, csrc/incres.hip; the contract is DESIGN.md 4.15): the transition matrix P
    as CSR arrays whose rows keep their STORED order (scipy's `W*D`, unsorted, as it is) and a state of k columns that stays on the
    device.  step(seeds, max_grow) plants the (k, m) seeds, grows until no entry of the state is zero and returns (labels (n) int32,
    sweeps).  A context manager; close() releases the device memory.  GlxError on every refusal of the library, the cap on the sweeps
    included; the object stays usable after it (`last_sweeps` then holds the cap)."""

    _destroy = 'glx_incres_destroy'

    def __init__(self, row_ptr, col, val, k, device=None):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        n = len(row_ptr) - 1
        if row_ptr.ndim != 1 or n < 1 or col.ndim != 1 or val.shape != col.shape or int(row_ptr[0]) != 0 or int(row_ptr[-1]) != len(col):
            raise GlxError('Incres: inconsistent array shapes or sizes')
        self.n, self.k = n, int(k)
        self.last_sweeps = None
        self._open('glx_incres_create', n, _ptr(row_ptr), _ptr(col), _ptr(val), int(k), _dev(device))

    def step(self, seeds, max_grow=None, out=None):
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        if seeds.ndim != 2 or seeds.shape[0] != self.k or seeds.shape[1] < 1:
            raise GlxError('Incres.step: seeds of shape %s, expected (%d, m >= 1)' % (seeds.shape, self.k))
        labels = pinned_empty((self.n,), np.int32) if out is None else out
        if labels.dtype != np.int32 or labels.shape != (self.n,) or not labels.flags.c_contiguous:
            raise GlxError('Incres.step: out must be a contiguous int32 array of %d entries' % self.n)
        sweeps = C.c_int64(-1)
        self.last_sweeps = None
        rc = load().glx_incres_step(self._handle(), _ptr(seeds), seeds.shape[1], int(2 * self.n + 2 if max_grow is None else max_grow),
                                    _ptr(labels), C.byref(sweeps))
        self.last_sweeps = int(sweeps.value)
        check(rc, 'glx_incres_step')
        return labels, int(sweeps.value)

    def stats(self):
        """dict: chunk_cap, first_chunk, margin, next_chunk, loops, chunks, enqueued, counted, lanes, record, renumbered, slices"""
        out = (C.c_int64 * 12)()
        call('glx_incres_stats', self._handle(), out)
        names = ('chunk_cap', 'first_chunk', 'margin', 'next_chunk', 'loops', 'chunks', 'enqueued', 'counted', 'lanes', 'record', 'renumbered',
                 'slices')
        return dict(zip(names, (int(v) for v in out)))


ACQ_VAR, ACQ_SIGMA, ACQ_MC, ACQ_MCVAR = 0, 1, 2, 3          # the kinds of glx_acq_compute (include/glx_experimental.h)
ACQ_MAX_M = 256


class Acq(_Handle):
    """The device half of the acquisition functions of active learning (glx_acq_*, csrc/acq.hip; the contract is DESIGN.md 4.19): the
    eigenvectors V (n, M) and the covariance C (M, M) stay on the device.  compute(kind, cand, unc) evaluates the candidates,
    update(query) applies the rank-one steps of a batch in one launch, greedy(kind, cand, b) returns the positions in cand and the
    values that b rounds of evaluate / take the first maximum / update choose, on a scratch copy of C.  A context manager; close()
    releases the device memory.  GlxError on every refusal of the library; the object stays usable after it."""

    _destroy = 'glx_acq_destroy'

    def __init__(self, V, C_, gamma2, device=None):
        V = np.ascontiguousarray(V, dtype=np.float64)
        C_ = np.ascontiguousarray(C_, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 1 or C_.shape != (V.shape[1], V.shape[1]):
            raise GlxError('Acq: V of shape %s and C of shape %s, expected (n, M) and (M, M)' % (V.shape, C_.shape))
        self.n, self.M = V.shape
        self._open('glx_acq_create', self.n, self.M, _ptr(V), _ptr(C_), float(gamma2), _dev(device))

    def compute(self, kind, cand, unc=None):
        cand = np.ascontiguousarray(cand, dtype=np.int32).ravel()
        if unc is not None:
            unc = _dense(np.asarray(unc).ravel(), np.float64, (len(cand),), 'unc')
        vals = np.empty(len(cand), dtype=np.float64)
        call('glx_acq_compute', self._handle(), int(kind), _ptr(cand), len(cand), _ptr(unc), _ptr(vals))
        return vals

    def update(self, query):
        query = np.ascontiguousarray(query, dtype=np.int32).ravel()
        call('glx_acq_update', self._handle(), _ptr(query), len(query))

    def greedy(self, kind, cand, b):
        """(positions in cand (b) int32, their values (b))"""
        cand = np.ascontiguousarray(cand, dtype=np.int32).ravel()
        b = int(b)
        queries = np.empty(max(b, 1), dtype=np.int32)
        vals = np.empty(max(b, 1), dtype=np.float64)
        call('glx_acq_greedy', self._handle(), int(kind), _ptr(cand), len(cand), b, _ptr(queries), _ptr(vals))
        return queries[:b], vals[:b]

    def get_c(self):
        out = np.empty((self.M, self.M), dtype=np.float64)
        call('glx_acq_get_c', self._handle(), _ptr(out))
        return out

    def stats(self):
        """dict: pass_launches, update_launches, greedy_launches, tile_rows, pass_lds, update_lds, n, M"""
        out = (C.c_int64 * 8)()
        call('glx_acq_stats', self._handle(), out)
        names = ('pass_launches', 'update_launches', 'greedy_launches', 'tile_rows', 'pass_lds', 'update_lds', 'n', 'M')
        return dict(zip(names, (int(v) for v in out)))


def host_row_sums(W):
    """W * ones for a CSR matrix with int32 indices (scipy's csr_matvec order), by the library's host loop."""
    out = np.empty(W.shape[0], dtype=np.float64)
    call('glx_host_row_sums', W.shape[0], _ptr(W.indptr), _ptr(W.data), _ptr(out))
    return out


def host_neg_columns_rows(Lcsc, cols, F, row_scale=None):
    """(rows ascending int32, values (len(rows), k)) of -L[:, cols] * F without the rows in `cols`, each row times row_scale[row]
    (glx_host_neg_columns_rows: csr_matvecs' order of a row's terms); None when the preconditions do not hold (the caller then
    takes the literal expression)."""
    n = Lcsc.shape[0]
    cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
    F = np.ascontiguousarray(F, dtype=np.float64)
    if Lcsc.indptr.dtype != np.int32 or Lcsc.indices.dtype != np.int32 or Lcsc.data.dtype != np.float64 or F.ndim != 2 or len(F) != len(cols):
        return None
    if len(cols) and (cols.min() < 0 or cols.max() >= n):
        return None
    k = F.shape[1]
    cap = int(Lcsc.indptr[cols + 1].astype(np.int64).sum() - Lcsc.indptr[cols].astype(np.int64).sum()) if len(cols) else 0
    rows = np.empty(max(cap, 1), dtype=np.int32)
    vals = np.empty((max(cap, 1), k), dtype=np.float64)
    cnt = C.c_int64(0)
    scale = None if row_scale is None else np.ascontiguousarray(row_scale, dtype=np.float64)
    call('glx_host_neg_columns_rows', n, _ptr(Lcsc.indptr), _ptr(Lcsc.indices), _ptr(Lcsc.data), len(cols), _ptr(cols), _ptr(F), k, _ptr(scale), cap,
         _ptr(rows), _ptr(vals), C.byref(cnt))
    if cnt.value < 0:
        return None
    return rows[:cnt.value], vals[:cnt.value]


def host_reverse_scale_rows(W, scale):
    """(indices, data) of the matrix whose row i is row i of W times scale[i] with the entries in reverse order."""
    col = np.empty(W.nnz, dtype=np.int32)
    val = np.empty(W.nnz, dtype=np.float64)
    call('glx_host_reverse_scale_rows', W.shape[0], _ptr(W.indptr), _ptr(W.indices), _ptr(W.data), _ptr(scale), _ptr(col), _ptr(val))
    return col, val


def auto_cells(n, d):
    """How many cells glx_knn_clustered forms when the caller leaves it to the library: none below 2^17 rows (the all-pairs
    search takes a few ms there) or above 128 features (the cell pruning rides on the split-bf16 filter), else one per 8192
    rows within [16, 256].  GLX_KNN_CLUSTERED=0 turns it off, =<m> forces m cells."""
    e = os.environ.get('GLX_KNN_CLUSTERED')
    if e is not None:
        return max(0, int(e))
    if n < (1 << 17) or d > 128:
        return 0
    return int(min(256, max(64, n // 8192)))      # (>= 64: the cells' order also serves as the vertex order of the graph's operators)


def auto_order_cells(n, d):
    """Below the size of the cell-PRUNED search: how many chained cells the rows are reordered by before the all-pairs search
    (coherent wavefronts: 10-14 % of the search on clustered data, nothing lost elsewhere), whose order the operators on the
    graph then take instead of their own pass over the graph (3.7 ms at 70 000 vertices).  GLX_KNN_ORDER=0 turns it off."""
    if os.environ.get('GLX_KNN_ORDER', '1') == '0' or n < 4096 or n >= (1 << 17) or d > 128:
        return 0
    return int(min(128, n // 64))     # (measured at 70 000 x 20: 128 cells = the library's order to 0.5 %, 64 and 32 cells 0.5-1 % behind)


class _KnnOptions(C.Structure):
    _fields_ = [('filter', C.c_int), ('lists', C.c_int), ('nsplit', C.c_int), ('concat', C.c_int)]


class knn_options:
    """Context manager: plan overrides for the calling thread's kNN searches (glx_knn_set_options) -- which candidate filter
    ('bf16' | 'f32'), list length ('short' | 'long'), ref ranges per query block (1..8; 1..32 for k > 60), operand form of the bf16 filter at
    d <= 21 (concat 0 | 1 | 2).  Every plan returns the same exact lists; tests and A/B measurements use this."""

    def __init__(self, filter=None, lists=None, nsplit=None, concat=None):
        self.opt = _KnnOptions({None: 0, 'bf16': 1, 'f32': 2}[filter], {None: 0, 'short': 1, 'long': 2}[lists],
                                int(nsplit or 0), -1 if concat is None else int(concat))

    def __enter__(self):
        call('glx_knn_set_options', C.byref(self.opt))
        return self

    def __exit__(self, *exc):
        load().glx_knn_set_options(None)
        return False


def _knn_input(X, similarity):
    X = np.asarray(X, dtype=np.float64)
    if similarity == 'angular':
        X = X / np.linalg.norm(X, axis=1)[:, None]
    elif similarity != 'euclidean':
        raise GlxError('similarity %r not supported (euclidean, angular)' % (similarity,))
    return np.ascontiguousarray(X)


def _knn_cells(n, d, clustered, want_order):
    """The `ncells` argument of glx_knn_clustered / glx_knn_search for a full search."""
    m = auto_cells(n, d) if clustered is None else int(clustered)
    if m <= 1 and clustered is None and want_order and auto_order_cells(n, d) > 1:
        m = -auto_order_cells(n, d)     # all pairs on rows reordered by that many chained cells
    return m if (m > 1 or m < -1) else 0


def knn_bruteforce(X, k, similarity='euclidean', device=None, query_range=None, cell_starts=None, clustered=None, want_order=False):
    """Exact kNN (incl. self, k <= KNN_K_LISTS; KnnResult takes more) on the GPU.  'angular' = euclidean on row-normalised data, formed
    with the reference's own expression (weightmatrix.py:344-345).  cell_starts: the rows come in a coarse geometric
    order with cell c = rows [cell_starts[c], cell_starts[c+1]); the search skips the cells that cannot hold a
    neighbour (glx_knn_cells_range: the same lists, a fraction of the tiles on clustered data).  clustered: number of cells
    the library forms itself (glx_knn_clustered; None = auto_cells(n, d), 0 = all pairs).
    want_order (below the size of the pruned search): the rows are put into the order of chained cells before the search
    (coherent wavefronts; a plain knnsearch does not ask: 0.1 ms at d = 20, 0.7 ms at d = 128 for 50 000 rows) -- KnnResult
    hands that order out as well."""
    dev_ptr = None
    if hasattr(X, 'data_ptr') and getattr(X, 'is_cuda', False):
        # a torch CUDA tensor (float64, contiguous, euclidean): the search reads it where it is (range / cells forms only)
        if similarity != 'euclidean' or str(X.dtype) != 'torch.float64' or not X.is_contiguous() or (query_range is None and cell_starts is None):
            raise GlxError('a device-resident X must be a contiguous float64 tensor, euclidean, searched by range or by cells')
        n, d = int(X.shape[0]), int(X.shape[1])
        dev_ptr = _vp(X.data_ptr())
    else:
        X = _knn_input(X, similarity)
        n, d = X.shape
    q0, q1 = (0, n) if query_range is None else query_range
    ind = pinned_empty((q1 - q0, k), np.int64)       # page-locked result arrays: the copy back runs at PCIe speed
    dist = pinned_empty((q1 - q0, k), np.float64)
    if cell_starts is not None:
        cs = np.ascontiguousarray(cell_starts, dtype=np.int64)
        call('glx_knn_cells_range', dev_ptr or _ptr(X), n, d, k, _ptr(cs), len(cs), q0, q1, _ptr(ind), _ptr(dist), _dev(device))
        return ind, dist
    if dev_ptr is not None:
        call('glx_knn_bruteforce_range', dev_ptr, n, d, k, q0, q1, _ptr(ind), _ptr(dist), _dev(device))
        return ind, dist
    m = _knn_cells(n, d, clustered, want_order) if query_range is None else 0
    if m:       # cells formed by the library (same lists; a fraction of the tiles when the data has clusters)
        call('glx_knn_clustered', _ptr(X), n, d, k, m, _ptr(ind), _ptr(dist), _dev(device))
        return ind, dist
    call('glx_knn_bruteforce_range', _ptr(X), n, d, k, q0, q1, _ptr(ind), _ptr(dist), _dev(device))
    return ind, dist


_PINNED_CSR_MAX = 512 << 20      # above this the weight matrix comes back through ordinary memory
_KERNEL_ID = {'given': 0, 'uniform': 1, 'gaussian': 2, 'symgaussian': 3, 'distance': 4, 'singular': 5}


KNN_K_LISTS = 60      # k (self included) of the list-returning searches: knn_bruteforce and the sharded build
KNN_K_MAX = 1024      # k (self included) of KnnResult (glx_knn_search)


class KnnResult(_Handle):
    """A finished full search whose lists live on the device (glx_knn_search): `to_csr` builds the weight matrix from them
    without a host round trip, `lists()` copies them out, `order()` is the cell order the search worked out (or None).
    k (self included) from 1 to min(n, KNN_K_MAX); above KNN_K_LISTS the search takes its wide plan (longer and more
    candidate lists, processed in chunks of queries), whose lists are the same exact lists."""

    _destroy = 'glx_knn_result_destroy'

    def __init__(self, X, k, similarity='euclidean', device=None, clustered=None, want_order=False):
        X = _knn_input(X, similarity)
        n, d = X.shape
        self.n, self.k, self.device = n, int(k), _dev(device)
        self._open('glx_knn_search', _ptr(X), n, d, int(k), _knn_cells(n, d, clustered, want_order), self.device)

    def lists(self):
        ind = pinned_empty((self.n, self.k), np.int64)
        dist = pinned_empty((self.n, self.k), np.float64)
        call('glx_knn_result_lists', self._handle(), _ptr(ind), _ptr(dist))
        return ind, dist

    def order(self):
        perm = pinned_empty((self.n,), np.int32)         # (a device-to-host copy into fresh pageable memory takes milliseconds the first time)
        if load().glx_knn_result_order(self._handle(), _ptr(perm)) != 0:
            return None
        return perm

    def to_csr(self, k, kernel='gaussian', sym=1, weights=None):
        from scipy import sparse
        n = self.n
        w = None if weights is None else _dense(weights, np.float64, (n, k), 'weights')
        cap = n * int(k) * (2 if sym else 1)
        pinned = cap * 12 <= _PINNED_CSR_MAX
        indptr = pinned_empty((n + 1,), np.int32) if pinned else np.empty(n + 1, np.int32)
        col_buf = pinned_empty((cap,), np.int32) if pinned else np.empty(cap, np.int32)
        val_buf = pinned_empty((cap,), np.float64) if pinned else np.empty(cap, np.float64)
        nnz = C.c_int64(0)
        call('glx_knn_result_to_csr', self._handle(), int(k), _KERNEL_ID[kernel], int(sym), _ptr(w), cap, _ptr(indptr), _ptr(col_buf), _ptr(val_buf),
             C.byref(nnz))
        W = sparse.csr_matrix((val_buf[:nnz.value], col_buf[:nnz.value], indptr), shape=(n, n))
        W.has_sorted_indices = True
        W.has_canonical_format = True
        return W


class BallResult(_Handle):
    """A finished radius search whose structure lives on the device (glx_ball_search): `to_csr` weighs it and returns the
    scipy CSR matrix, `structure()` returns it with the distances the weights see instead (for kernels evaluated on the host)."""

    _destroy = 'glx_ball_result_destroy'

    def __init__(self, X, epsilon, features=None, device=None):
        X = _dense(X, np.float64, name='data')
        n, d = X.shape
        F = None if features is None else _dense(features, np.float64, name='features')
        if F is not None and (F.ndim != 2 or F.shape[0] != n):
            raise GlxError('features have shape %s, expected (%d, m)' % (F.shape, n))
        self.n, self.device, self.has_features = n, _dev(device), F is not None
        self._open('glx_ball_search', _ptr(X), n, d, float(epsilon), _ptr(F), 0 if F is None else F.shape[1], self.device)
        nnz = C.c_int64(0)
        call('glx_ball_result_nnz', self._handle(), C.byref(nnz))
        self.nnz = nnz.value

    def _arrays(self, specs):
        pinned = sum(int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in specs) <= _PINNED_CSR_MAX
        return [(pinned_empty(shape, dt) if pinned else np.empty(shape, dt)) for shape, dt in specs]

    def _csr(self, indptr, col, val, m):
        from scipy import sparse
        if 2 * m < self.nnz:        # zero weights were dropped: a view would keep the full-size (page-locked) block alive behind it
            val, col = val[:m].copy(), col[:m].copy()
        W = sparse.csr_matrix((val[:m], col[:m], indptr), shape=(self.n, self.n))
        W.has_sorted_indices = True
        W.has_canonical_format = True
        return W

    def to_csr(self, kernel='gaussian', epsilon_f=1.0):
        """The weight matrix of one of the device kernels ('uniform', 'gaussian', 'distance', 'singular'), zero weights dropped."""
        indptr, col, val = self._arrays([((self.n + 1,), np.int32), ((self.nnz,), np.int32), ((self.nnz,), np.float64)])
        m = C.c_int64(0)
        call('glx_ball_result_to_csr', self._handle(), _KERNEL_ID[kernel], float(epsilon_f), _ptr(indptr), _ptr(col), _ptr(val), None, None,
             C.byref(m))
        return self._csr(indptr, col, val, m.value)

    def structure(self):
        """(indptr, indices, dists, fdists): the rows (ascending columns, nothing dropped) and, entry by entry, the squared
        distance in numpy's summation order and the squared feature distance (None without features)."""
        specs = [((self.n + 1,), np.int32), ((self.nnz,), np.int32), ((self.nnz,), np.float64)]
        if self.has_features:
            specs.append(((self.nnz,), np.float64))
        arrs = self._arrays(specs)
        indptr, col, dists = arrs[:3]
        fd = arrs[3] if self.has_features else None
        m = C.c_int64(0)
        call('glx_ball_result_to_csr', self._handle(), _KERNEL_ID['given'], 1.0, _ptr(indptr), _ptr(col), None, _ptr(dists), _ptr(fd), C.byref(m))
        return indptr, col[:m.value], dists[:m.value], (None if fd is None else fd[:m.value])


def ball_stats():
    out = (C.c_double * 8)()
    call('glx_ball_stats', out)
    return dict(pairs_tested=out[0], pairs_accepted=out[1], cells=int(out[2]), grid_ms=out[3], count_ms=out[4], fill_ms=out[5],
                sort_ms=out[6], weights_ms=out[7])


def exp_cr(x, device=None):
    """exp(x), correctly rounded, evaluated on the device (glx_exp_cr)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    call('glx_exp_cr', _ptr(x), _ptr(out), x.size, _dev(device))
    return out


def knn_to_csr(knn_ind, knn_dist, k, kernel='gaussian', sym=1, weights=None, device=None):
    """kNN data -> scipy CSR weight matrix, assembled on the GPU (glx_knn_to_csr)."""
    from scipy import sparse
    ind = np.ascontiguousarray(knn_ind, dtype=np.int64)
    n, kk = ind.shape
    # distances are only read by the kernels that compute weights from them: with given weights they need not travel
    dist = None if (knn_dist is None or kernel == 'given') else _dense(knn_dist, np.float64, (n, kk), 'knn_dist')
    w = None if weights is None else _dense(weights, np.float64, (n, k), 'weights')
    nnz = C.c_int64(0)
    lib = load()
    cap = n * int(k) * (2 if sym else 1)                   # every list entry appears at most twice (as i->j and as j->i)
    if cap * 12 <= _PINNED_CSR_MAX:
        # the CSR lands in page-locked arrays of the pool (recycled by size: the next graph of the same (n, k) reuses them);
        # indices / data are views of the first nnz entries
        indptr = pinned_empty((n + 1,), np.int32)
        col_buf = pinned_empty((cap,), np.int32)
        val_buf = pinned_empty((cap,), np.float64)
        call('glx_knn_to_csr_into', _ptr(ind), _ptr(dist), _ptr(w), n, kk, int(k), _KERNEL_ID[kernel], int(sym), cap, _ptr(indptr), _ptr(col_buf),
             _ptr(val_buf), C.byref(nnz), _dev(device))
        indices, data = col_buf[:nnz.value], val_buf[:nnz.value]
    else:
        rp, ci, va = _vp(), _vp(), _vp()
        call('glx_knn_to_csr', _ptr(ind), _ptr(dist), _ptr(w), n, kk, int(k), _KERNEL_ID[kernel], int(sym), C.byref(rp), C.byref(ci), C.byref(va),
             C.byref(nnz), _dev(device))
        try:
            m = nnz.value
            indptr = np.ctypeslib.as_array(C.cast(rp, _i32p), shape=(n + 1,)).copy()
            indices = np.ctypeslib.as_array(C.cast(ci, _i32p), shape=(max(m, 1),))[:m].copy()
            data = np.ctypeslib.as_array(C.cast(va, _f64p), shape=(max(m, 1),))[:m].copy()
        finally:
            lib.glx_free(rp)
            lib.glx_free(ci)
            lib.glx_free(va)
    W = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    W.has_sorted_indices = True
    W.has_canonical_format = True
    return W


def knn_rows_to_csr(J_own, w_own, n_cols, row_base, rev_row, rev_src, rev_pos, rev_w, sym=1, device=None):
    """Rows [row_base, row_base + m) of weightmatrix.knn's matrix from the block's own lists and the reverse entries sent by the
    owners of the other rows, merged on the GPU (glx_knn_rows_to_csr).  Returns a scipy CSR of shape (m, n_cols)."""
    from scipy import sparse
    J = np.ascontiguousarray(J_own, dtype=np.int64)
    m, k = J.shape
    w = _dense(w_own, np.float64, (m, k), 'w_own')
    rr = np.ascontiguousarray(rev_row, dtype=np.int64)
    rs = np.ascontiguousarray(rev_src, dtype=np.int64)
    rp = np.ascontiguousarray(rev_pos, dtype=np.int64)
    rw = np.ascontiguousarray(rev_w, dtype=np.float64)
    cap = m * k + len(rr)
    indptr = np.empty(m + 1, dtype=np.int32)
    col = np.empty(max(cap, 1), dtype=np.int32)
    val = np.empty(max(cap, 1), dtype=np.float64)
    nnz = C.c_int64(0)
    call('glx_knn_rows_to_csr', _ptr(J), _ptr(w), m, k, int(n_cols), int(row_base), _ptr(rr), _ptr(rs), _ptr(rp), _ptr(rw), len(rr), int(sym), cap,
         _ptr(indptr), _ptr(col), _ptr(val), C.byref(nnz), _dev(device))
    W = sparse.csr_matrix((val[:nnz.value].copy(), col[:nnz.value].copy(), indptr), shape=(m, int(n_cols)))
    W.has_sorted_indices = True
    W.has_canonical_format = True
    return W


def host_locality_order(indptr, indices, col_lo=0):
    """perm[new] = old: the library's breadth-first locality order of an n-row pattern restricted to columns [col_lo, col_lo + n)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    n = len(indptr) - 1
    perm = np.empty(n, dtype=np.int32)
    call('glx_host_locality_order', n, _ptr(indptr), _ptr(indices), int(col_lo), _ptr(perm))
    return perm


def host_permute_rows(A, perm):
    """csr_matrix with row i = row perm[i] of A (entry order inside the rows kept), on host threads."""
    from scipy import sparse
    indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(A.indices, dtype=np.int32)
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    perm = np.ascontiguousarray(perm, dtype=np.int64)
    n = len(indptr) - 1
    ip, ix, dv = np.empty(n + 1, dtype=np.int32), np.empty(len(indices), dtype=np.int32), np.empty(len(data), dtype=np.float64)
    call('glx_host_permute_rows', n, _ptr(indptr), _ptr(indices), _ptr(data), _ptr(perm), _ptr(ip), _ptr(ix), _ptr(dv))
    out = sparse.csr_matrix((dv, ix, ip), shape=A.shape)
    out.has_sorted_indices = A.has_sorted_indices
    return out


def knn_stats():
    out = (C.c_double * 16)()
    call('glx_knn_stats', out)
    return dict(tile_ms=out[0], rerank_ms=out[1], fallback_rows=out[2], total_ms=out[3], fallback_ms=out[4],
                dpa=out[5], nsplit=out[6], KP=abs(out[7]), filter='bf16x3' if out[7] < 0 else 'f32', escalated_rows=out[8],
                concatenated=int(out[9]), seed_sample=int(out[10]), visited_share=out[11], cells=int(out[12]),
                chunks=int(out[13]), wide=bool(out[14]), candidates=int(out[15]))
