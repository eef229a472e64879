"""ctypes binding of libvoxproj.so (the C-ABI declared in include/voxproj.h) plus workspace plumbing.

PyTorch is used only for device memory and streams.  There is NO CPU fallback: if the HIP library is
missing or no GPU is visible, the product entry points raise.
"""
import collections
import ctypes
import os
import subprocess
import threading
import weakref

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VOXPROJ_LIB") or os.path.join(_HERE, "libvoxproj.so")

VP_OK = 0
VP_FLAG_SYNC = 1
VP_FLAG_REUSE_ACCEL = 2
VP_FLAG_EXACT_MARCH = 4
VP_FLAG_PIPELINE = 8
VP_FLAG_VERIFY_ACCEL = 16
VP_FLAG_SERIAL_SUMS = 32
VP_FLAG_GATHER_ONLY = 64

_lib = None
_lock = threading.Lock()

# test / A-B switches of the ctypes front (module attributes, not environment variables; the compiled front has
# project_features_cuda.set_exact_march / set_accel_cache)
EXACT_MARCH = False      # evaluate every ray sample like K.cu:47-82 (VP_FLAG_EXACT_MARCH)
ACCEL_CACHE = True       # keep the occupancy-derived tables between calls on the same, unmodified occupancy tensor
_default_options = {}    # {VP_OPT_*: value} applied to every Workspace of this module (set_default_option)
_options_version = 0


def set_default_option(option, value):
    """Default of a workspace option (VP_OPT_HEAVY_THRESHOLD, VP_OPT_MARCH_LDS_KB) for every Workspace object of this
    process, existing ones included (they pick it up at their next call); None = the library's default.  A Workspace's
    own set_option wins.  Test / A-B switch: production code leaves the defaults alone."""
    global _options_version
    if value is None:
        _default_options.pop(int(option), None)
    else:
        _default_options[int(option)] = int(value)
    _options_version += 1


# The C ABI of include/voxproj.h, one entry per function: "<return type>: <argument types>", one letter per type (the blanks
# only group runs).  Pointers to device memory, workspaces and streams are ``p``; the capital letters are the host arrays a
# caller passes as ctypes arrays.  tests/test_abi_cpu.py compares every entry with the header's prototype.
_C_TYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "q": ctypes.c_longlong, "u": ctypes.c_uint64,
            "z": ctypes.c_size_t, "f": ctypes.c_float, "d": ctypes.c_double, "s": ctypes.c_char_p,
            "F": ctypes.POINTER(ctypes.c_float), "D": ctypes.POINTER(ctypes.c_double),
            "I": ctypes.POINTER(ctypes.c_int32), "L": ctypes.POINTER(ctypes.c_int64)}
_SIGNATURES = {
    # ABI version 4
    "vp_abi_version": "i:",
    "vp_last_error": "s:",
    "vp_workspace_bytes": "z: iiiiiiii l",
    "vp_project_features": "i: pppp F ppp F f iiiiiiii l p z p i",
    "vp_project_features_f16": "i: pppp F ppp F f iiiiiiii l p z p i",
    "vp_workspace_status": "i: pp",
    "vp_workspace_counters": "i: p I i p",
    "vp_copy_hit_image": "i: pp iiiiiiii l p",
    "vp_profile_enable": "i: i",
    "vp_profile_read": "i: D L",
    "vp_workspace_release": "i: p",
    "vp_workspace_create": "i: p z",
    "vp_workspace_set_option": "i: p i q",
    "vp_workspace_table_builds": "q: p",
    "vp_project_colors": "i: p iii pp i F d p ii pppp l i p z p",
    "vp_colors_workspace_bytes": "z: l",
    "vp_nearest_voxel": "i: ppp D d iii p l pp",
    "vp_stream_read": "i: p l pp",
    "vp_upsample_workspace_bytes": "z: iiii",
    "vp_upsample_features": "i: p iiii p iii p z p",
    "vp_voxel_coords": "i: p l F f pp I p",
    "vp_scatter_occupancy": "i: p l I iii ppp",
    "vp_aggregate_view_f16": "i: ppppp i p l i p",
    "vp_first_hit_ids": "i: ppp FF f iiiiiii l pp z p i",
    "vp_render_features": "i: p l p l i p i pp",
    "vp_query_workspace_bytes": "z: ii",
    "vp_query_features": "i: p i l i l p i f ppppp z p",
    "vp_splat_workspace_bytes": "z: l ii l",
    "vp_splat_project": "i: pppp l F ffff ii fff ppp z p",
    "vp_splat_rasterize": "i: p i ll ii l pppppp z p",
    "vp_splat_backward_workspace_bytes": "z: l i",
    "vp_splat_rasterize_backward": "i: p i ll ii l pppppp z p z p",
    "vp_splat_geometry_backward_workspace_bytes": "z: l i",
    "vp_splat_rasterize_backward_geometry": "i: pppp i ll F ffff ii f l pppppppppp z p z p",
    "vp_splat_loss_workspace_bytes": "z: ii",
    "vp_splat_rasterize_loss": "i: p i ll ii l pppppppppp z p z p",
    "vp_splat_loss_backward": "i: pppp i ll F ffff ii f l pppp i pppppppppp z p z p",
    "vp_label_scores_workspace_bytes": "z: ii",
    "vp_label_boundary": "i: p iii pp z p",
    "vp_label_scores": "i: pp iiii ppppp z p",
    # added after ABI version 4: a library may lack them (detected by symbol; _entry raises for a missing one)
    "vp_splat_lift_workspace_bytes": "z: l i",
    "vp_splat_lift": "i: p i l p l ii l i p l ppp z p z p",
    "vp_splat_render": "i: p ii ll ii l i p i l ppp z p",
    "vp_feature_loss_workspace_bytes": "z: ii",
    "vp_feature_loss": "i: p i l p l iii pp f i ppp z p",
    "vp_feature_loss_gradient": "i: p i l p l iii p i pp l pp z p",
    "vp_proto_contrast_workspace_bytes": "z: iii",
    "vp_proto_contrast": "i: p iii pp ii fff pppp z p",
    "vp_proto_contrast_gradient": "i: p iii pp ff ppp z p",
    "vp_codebook_workspace_bytes": "z: iiii",
    "vp_codebook_assoc": "i: p iii p i p i pppp z p",
    "vp_codebook_loss": "i: p iii p i p f p i pppppp z p",
    "vp_knn_points": "i: ppp D d iii pp l i ppp",
    "vp_neighbor_kl_workspace_bytes": "z: l",
    "vp_neighbor_kl": "i: p l i l p l p i ppp i p z p",
    "vp_neighbor_kl_gradient": "i: p l i l p l p i ppppp d pp l i p",
    "vp_photo_loss_workspace_bytes": "z: iii",
    "vp_photo_loss": "i: pp iii ppp z p",
    "vp_photo_loss_gradient": "i: pp iii f ppp z p",
    "vp_densify_accumulate": "i: p l ii f pppp fffff pppp z p",
    "vp_densify_plan_workspace_bytes": "z: l",
    "vp_densify_plan": "i: ppppp l fffff pppp z p",
    "vp_densify_rows": "i: p i ppp ll pp",
    "vp_densify_split": "i: ppp l ppp l u pppp",
}
EXPORTS = list(_SIGNATURES)
VP_ABI_VERSION = 4
# The entry points of include/voxproj_ext.h, added after the 64 above (which are frozen with voxproj.h): the same notation, the
# same tolerant binding and the same _call helper.  tests/test_sh_cpu.py compares every entry with that header's prototype.
_SIGNATURES_EXT = {
    "vp_sh_colors": "i: ppp F l ii pp p",
    "vp_sh_colors_backward": "i: ppp F l ii pp ppp p",
}
EXPORTS_EXT = list(_SIGNATURES_EXT)
# The entry points of include/voxproj_mesh.h (the triangle-mesh rasterizer): the third table, same notation, same tolerant
# binding.  tests/test_mesh_cpu.py compares every entry with that header's prototype.
_SIGNATURES_MESH = {
    "vp_mesh_workspace_bytes": "z: l ii l",
    "vp_mesh_project": "i: p l p l F ffff ii ff pp p z p",
    "vp_mesh_rasterize": "i: pp l ii l pppp p z p",
}
EXPORTS_MESH = list(_SIGNATURES_MESH)
# The entry points of include/voxproj_grid.h (stage 2, the voxel grid of a Gaussian cloud): the fourth table, same notation,
# same tolerant binding.  tests/test_voxel_grid_cpu.py compares every entry with that header's prototype.
_SIGNATURES_GRID = {
    "vp_ball_count": "i: ppp D d iii p l d ppp d pp p",
    "vp_voxel_grid_workspace_bytes": "z: l",
    "vp_voxel_grid": "i: ppp l d ppppp ppp p z p",
}
EXPORTS_GRID = list(_SIGNATURES_GRID)
# The entry points of include/voxproj_cluster.h (label sums over a feature table, the rows' inverse norms): the fifth table, same
# notation, same tolerant binding.  tests/test_label_sums_cpu.py compares every entry with that header's prototype.
_SIGNATURES_CLUSTER = {
    "vp_row_inv_norms": "i: p i l i l pp p",
    "vp_label_sums_workspace_bytes": "z: l ii",
    "vp_label_sums": "i: p i l i l pp i l ppp p z p",
}
EXPORTS_CLUSTER = list(_SIGNATURES_CLUSTER)
VP_SH_MAX_DEGREE = 3
VP_OPT_HEAVY_THRESHOLD = 1
VP_OPT_MARCH_LDS_KB = 2
VP_OPT_ROW_BEGIN = 3
VP_OPT_ROW_END = 4
VP_OPT_ONE_VIEW_GATHER = 5
VP_OPT_PART_PIXELS = 6
VP_OPT_ONE_VIEW_SPLIT = 7
VP_LOSS_SUM = 0
VP_LOSS_MEAN = 1
VP_FEATURE_LOSS_COSINE = 0
VP_FEATURE_LOSS_L2 = 1
VP_DENSIFY_MAX_ARRAYS = 16
VP_DENSIFY_MAX_WIDTH = 4096
VP_DENSIFY_COPY = 0
VP_DENSIFY_ZERO = 1


class VoxprojError(RuntimeError):
    pass


def build(force=False):
    """Compile libvoxproj.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f == "voxproj.hip" or (f.startswith("vp_") and f.endswith(".h"))]
    srcs += [os.path.join(os.path.dirname(_HERE), "include", h) for h in ("voxproj.h", "voxproj_ext.h", "voxproj_mesh.h", "voxproj_grid.h",
                                                                                   "voxproj_cluster.h")]
    newest = max(os.path.getmtime(f) for f in srcs)
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < newest:
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s"] + (["-B"] if force else []))
    return LIB_PATH


def ext_path():
    """Where ``setup.py build_ext --inplace`` puts the compiled drop-in module ``project_features_cuda``."""
    import sysconfig
    return os.path.join(_HERE, "project_features_cuda" + sysconfig.get_config_var("EXT_SUFFIX"))


def build_ext(force=False):
    """Build the compiled drop-in module with the package's setup.py (the counterpart of the reference's
    ``python setup.py install`` step, cuda_project_image_to_sparse_voxel/setup.py:10-27), in-tree: csrc/Makefile compiles
    the HIP kernels into libvoxproj.so, torch's BuildExtension compiles csrc/project_features_ext.cpp and links it to that
    library.  Returns the module's path."""
    import sys
    build(force)
    out = ext_path()
    src = os.path.join(_HERE, "csrc", "project_features_ext.cpp")
    hdr = os.path.join(os.path.dirname(_HERE), "include", "voxproj.h")
    newest = max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(os.path.join(_HERE, "setup.py")))
    if not force and os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    subprocess.check_call([sys.executable, "setup.py", "-q", "build_ext", "--inplace"] + (["--force"] if force else []), cwd=_HERE)
    return out


def lib():
    """Load the shared library (dlopen only; no device call is made here)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise VoxprojError(
                    f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                    "(there is no CPU fallback)")
            L = ctypes.CDLL(LIB_PATH)
            for name, signature in list(_SIGNATURES.items()) + list(_SIGNATURES_EXT.items()) + list(_SIGNATURES_MESH.items()) + \
                    list(_SIGNATURES_GRID.items()) + list(_SIGNATURES_CLUSTER.items()):
                fn = getattr(L, name, None)
                if fn is not None:               # a symbol the library lacks is skipped here; _entry raises when it is called
                    restype, argtypes = signature.split(":")
                    fn.restype = _C_TYPES[restype]
                    fn.argtypes = [_C_TYPES[c] for c in argtypes.replace(" ", "")]
            if L.vp_abi_version() != VP_ABI_VERSION:
                raise VoxprojError(f"{LIB_PATH} has ABI version {L.vp_abi_version()}, this package needs {VP_ABI_VERSION}: rebuild it")
            _lib = L
    return _lib


def last_error():
    return lib().vp_last_error().decode("utf-8", "replace")


def check(rc):
    if rc != VP_OK:
        raise VoxprojError(f"voxproj error {rc}: {last_error()}")


def _entry(name):
    """The library's function ``name``; a library built before it was added has none, and nothing stands in for it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise VoxprojError(f"{LIB_PATH} has no {name}: rebuild it (there is no fallback)")
    return fn


def _call(dev, name, *args):
    """Launch entry point ``name`` on ``dev``: the device made current, its current stream appended as the last argument,
    the return code checked."""
    import torch
    fn = _entry(name)
    with torch.cuda.device(dev):
        check(fn(*args, torch.cuda.current_stream(dev).cuda_stream))


def workspace_bytes(B, V, H, W, C, dimz, dimy, dimx, n_rows):
    return int(lib().vp_workspace_bytes(B, V, H, W, C, dimz, dimy, dimx, n_rows))


class Workspace:
    """Grow-only device scratch buffer (one per device), allocated through torch's allocator, announced to the library with
    vp_workspace_create and withdrawn with vp_workspace_release.  ``options``: {VP_OPT_*: value}, applied to every buffer
    this object ever holds (set_option)."""

    def __init__(self):
        self.buf = None
        self.accel_key = None     # (weakref to the occupancy tensor, its _version, shape, n_rows)
        self.options = {}
        self._applied = None      # (module options version, own options) last pushed to the library for self.buf

    def ensure(self, nbytes, device):
        import torch
        if self.buf is None or self.buf.numel() < nbytes + 256 or self.buf.device != device:
            if self.buf is not None:
                # growing while pipelined calls may be in flight: finish them before the old buffer goes away
                import torch as _t
                check(lib().vp_workspace_status(self.ptr(), _t.cuda.current_stream(self.buf.device).cuda_stream))
            self.release()
            self.buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
            self.accel_key = None
            check(lib().vp_workspace_create(self.ptr(), self.capacity()))      # whatever this address was before is forgotten
            self._applied = None
        self._push_options()
        return self.ptr()

    def _push_options(self):
        state = (_options_version, tuple(sorted(self.options.items())))
        if self.buf is None or self._applied == state:
            return
        merged = {VP_OPT_HEAVY_THRESHOLD: -1, VP_OPT_MARCH_LDS_KB: -1, VP_OPT_ROW_BEGIN: -1, VP_OPT_ROW_END: -1, VP_OPT_ONE_VIEW_GATHER: -1,
                  VP_OPT_PART_PIXELS: -1, VP_OPT_ONE_VIEW_SPLIT: -1}
        merged.update(_default_options)
        merged.update(self.options)
        for opt, val in merged.items():
            check(lib().vp_workspace_set_option(self.ptr(), int(opt), int(val)))
        self._applied = state

    def set_option(self, option, value):
        """vp_workspace_set_option (VP_OPT_HEAVY_THRESHOLD, VP_OPT_MARCH_LDS_KB); None = fall back to the module default /
        the library's.  Remembered, so it survives the buffer growing."""
        if value is None:
            self.options.pop(int(option), None)
        else:
            self.options[int(option)] = int(value)
        self._push_options()

    def set_row_range(self, begin=None, end=None):
        """Phase 2 of the following calls gathers only the voxel IDs in [begin, end) (VP_OPT_ROW_BEGIN / _END); no arguments:
        every row again.  With ``project_features_raw(..., gather_only=True)`` a call is cut into row ranges whose output rows
        are final one range after the other."""
        self.set_option(VP_OPT_ROW_BEGIN, begin)
        self.set_option(VP_OPT_ROW_END, end)

    def ptr(self):
        return (self.buf.data_ptr() + 255) & ~255

    def capacity(self):
        return self.buf.numel() - (self.ptr() - self.buf.data_ptr())

    def release(self):
        """Drop the library's side stream/events for this buffer (before the memory is recycled)."""
        if self.buf is not None and _lib is not None:
            _lib.vp_workspace_release(self.ptr())

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


_workspaces = {}


def get_workspace(device):
    """The ctypes front's per-device workspace (project_features_front.last_workspace covers both fronts)."""
    key = (device.type, device.index)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = Workspace()
    return ws


def project_features_raw(feats, occ, vmi, intr, opts5, count, out, grid_origin3, voxel_size,
                         workspace=None, sync=True, reuse_accel=None, exact_march=None, pipeline=False,
                         views_hit=None, verify_accel=False, gather_only=False, serial_sums=False, extra_flags=0):
    """Call vp_project_features (or vp_project_features_f16 when ``feats`` is float16) on torch CUDA tensors
    (already validated by the caller).

    opts5 / grid_origin3 are python sequences of floats.  Returns the Workspace used.
    ``reuse_accel``: None = reuse the occupancy-derived tables only if ``occ`` is the very same (still
    alive) tensor object as in the previous call on this workspace, with an unchanged torch version
    counter -- a data_ptr match alone is not enough, the caching allocator hands freed addresses out
    again; True/False = force.  ``exact_march``: evaluate every ray sample (A/B arm of the leaping march;
    default: module attribute EXACT_MARCH).  ``pipeline``: asynchronous job mode (VP_FLAG_PIPELINE): phase 1 of
    this call overlaps the previous call's gather; the caller must keep occ/vmi/intr alive and unchanged
    until ``workspace_status`` (or a device synchronise) and must not pass sync.  ``views_hit``: optional
    int32 [n_rows] tensor, += number of views of this call that hit each voxel.  ``verify_accel``: when the tables
    are not reused by identity (blocking calls only), let the library compare the grid with the copy the tables were
    built from and rebuild only if it changed (VP_FLAG_VERIFY_ACCEL) -- for callers that make a new, equal
    occupancy tensor for every call.  ``gather_only``: VP_FLAG_GATHER_ONLY -- no ray-march, phase 2 of the PREVIOUS call on
    this workspace (same tensors) once more, for the row range now set with ``Workspace.set_row_range``.
    ``serial_sums``: VP_FLAG_SERIAL_SUMS -- every voxel summed by one wavefront in (b, v, y, x) order, the oracle's bits (no
    workgroup path for voxels with very many pixels).
    """
    import torch
    B, V, H, W, C = feats.shape
    _, dimz, dimy, dimx = occ.shape
    n_rows = int(count.shape[0])
    ws = workspace if workspace is not None else get_workspace(feats.device)
    need = workspace_bytes(B, V, H, W, C, dimz, dimy, dimx, n_rows)
    ptr = ws.ensure(need, feats.device)
    key = (occ._version, occ.data_ptr(), tuple(occ.shape), n_rows)
    if reuse_accel is None:
        prev = ws.accel_key
        reuse_accel = (prev is not None and prev[0]() is occ and prev[1] == key and ACCEL_CACHE)
    if exact_march is None:
        exact_march = EXACT_MARCH
    flags = ((VP_FLAG_SYNC if (sync and not pipeline) else 0) | (VP_FLAG_REUSE_ACCEL if reuse_accel else 0)
             | (VP_FLAG_EXACT_MARCH if exact_march else 0) | (VP_FLAG_PIPELINE if pipeline else 0)
             | (VP_FLAG_VERIFY_ACCEL if (verify_accel and sync and not pipeline and not reuse_accel and ACCEL_CACHE) else 0)
             | (VP_FLAG_GATHER_ONLY if gather_only else 0) | (VP_FLAG_SERIAL_SUMS if serial_sums else 0) | int(extra_flags))
    o = (ctypes.c_float * 5)(*[float(v) for v in opts5])
    g = (ctypes.c_float * 3)(*[float(v) for v in grid_origin3])
    stream = torch.cuda.current_stream(feats.device).cuda_stream
    entry = lib().vp_project_features_f16 if feats.dtype == torch.float16 else lib().vp_project_features
    with torch.cuda.device(feats.device):
        rc = entry(
            feats.data_ptr(), occ.data_ptr(), vmi.data_ptr(), intr.data_ptr(), o,
            count.data_ptr(), out.data_ptr(), views_hit.data_ptr() if views_hit is not None else None,
            g, ctypes.c_float(float(voxel_size)),
            B, V, H, W, C, dimz, dimy, dimx, n_rows, ptr, ws.capacity(), stream, flags)
    if rc != VP_OK:
        ws.accel_key = None
        check(rc)
    ws.accel_key = (weakref.ref(occ), key)
    ws.last_shape = (B, V, H, W, C, dimz, dimy, dimx, n_rows)
    return ws


class PreparedViewCalls:
    """vp_project_features for a sequence of same-shaped calls on one scene, with everything that does not change between
    calls bound once (shapes, intrinsics, ray options, outputs, workspace, stream): the per-call work on the host is two
    pointer reads and one foreign call.  Used by the aggregator's one-view-per-call parity mode, where the kernels of a
    call run for ~0.2 ms and the general wrapper's Python would otherwise set the pace.  The first call builds the
    occupancy tables, the following ones reuse them (the caller keeps ``occ`` alive and unmodified meanwhile)."""

    def __init__(self, occ, intr, opts5, count, out, grid_origin3, voxel_size, workspace, shape, views_hit=None, flags=0):
        import torch
        self.B, self.V, self.H, self.W, self.C = (int(v) for v in shape)
        _, self.dimz, self.dimy, self.dimx = (int(v) for v in occ.shape)
        self.n_rows = int(count.shape[0])
        self.dev = occ.device
        self.keep = (occ, intr, count, out, views_hit)
        self.ws = workspace
        need = workspace_bytes(self.B, self.V, self.H, self.W, self.C, self.dimz, self.dimy, self.dimx, self.n_rows)
        self.ptr = workspace.ensure(need, self.dev)
        self.cap = workspace.capacity()
        self.o = (ctypes.c_float * 5)(*[float(v) for v in opts5])
        self.g = (ctypes.c_float * 3)(*[float(v) for v in grid_origin3])
        self.vs = ctypes.c_float(float(voxel_size))
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.fn32, self.fn16 = lib().vp_project_features, lib().vp_project_features_f16
        self.occ_ptr, self.intr_ptr = occ.data_ptr(), intr.data_ptr()
        self.count_ptr, self.out_ptr = count.data_ptr(), out.data_ptr()
        self.views_ptr = views_hit.data_ptr() if views_hit is not None else None
        self.flags = int(flags)
        self.built = False
        workspace.accel_key = None
        workspace.last_shape = (self.B, self.V, self.H, self.W, self.C, self.dimz, self.dimy, self.dimx, self.n_rows)

    def __call__(self, feats, vmi):
        """feats: CUDA tensor [B,V,H,W,C] (float32 or float16, contiguous), vmi: CUDA float32 [B*V*16]; asynchronous."""
        import torch
        if torch.cuda.current_device() != self.dev.index:
            torch.cuda.set_device(self.dev)       # the C-ABI works on the calling thread's current device
        fn = self.fn16 if feats.dtype == torch.float16 else self.fn32
        rc = fn(feats.data_ptr(), self.occ_ptr, vmi.data_ptr(), self.intr_ptr, self.o, self.count_ptr, self.out_ptr,
                self.views_ptr, self.g, self.vs, self.B, self.V, self.H, self.W, self.C, self.dimz, self.dimy, self.dimx,
                self.n_rows, self.ptr, self.cap, self.stream, self.flags | (VP_FLAG_REUSE_ACCEL if self.built else 0))
        if rc != VP_OK:
            self.built = False
            check(rc)
        self.built = True


def hit_image(ws, device):
    """First-hit ID image of the last call on ``ws`` as an int32 [B,V,H,W] tensor (test hook)."""
    import torch
    B, V, H, W, C, dimz, dimy, dimx, n_rows = ws.last_shape
    dst = torch.empty((B, V, H, W), dtype=torch.int32, device=device)
    ptr = ws.ptr()
    stream = torch.cuda.current_stream(device).cuda_stream
    check(lib().vp_copy_hit_image(ptr, dst.data_ptr(), B, V, H, W, C, dimz, dimy, dimx, n_rows, stream))
    torch.cuda.current_stream(device).synchronize()
    return dst


def _require(cond, msg):
    if not cond:
        raise ValueError(msg)


def _require_tensors(*specs):
    """(tensor, name, dtypes) triples: every dtype is checked first, then that each tensor is on a GPU."""
    import torch
    for t, name, dtypes in specs:
        _require(isinstance(t, torch.Tensor), f"{name} must be a torch tensor")
        _require(t.dtype in dtypes, f"{name} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    for t, name, _ in specs:
        _require(t.is_cuda, f"{name} must be a CUDA tensor: there is no CPU path")


def first_hit_ids(occ, vmi, intr, opts5, grid_origin3, voxel_size, H, W, n_rows, workspace=None, exact_march=None):
    """vp_first_hit_ids: the first-hit voxel ID of every pixel (0 = the ray hits nothing) for any cameras, without feature
    maps -- int32 [B,V,H,W], bit-identical to the hit image a forward call with the same arguments leaves.  occ int64
    [B,Z,Y,X], vmi float32 [B*V*16] camera->world, intr float32 [B,4], all on one CUDA device; opts5 / grid_origin3 python
    floats as for project_features_raw.  Blocking.  The tables built on ``workspace`` (default: this module's per-device one)
    are reused like project_features_raw reuses them."""
    import torch
    _require(len(opts5) == 5, "opts5 must hold 5 values: W, H, depth_min, depth_max, ray_increment")
    _require(len(grid_origin3) == 3, "grid_origin3 must hold 3 values")
    _require_tensors((occ, "occ", (torch.int64,)), (vmi, "vmi", (torch.float32,)), (intr, "intr", (torch.float32,)))
    _require(occ.dim() == 4 and occ.is_contiguous(), "occ must be a contiguous [B,Z,Y,X] tensor")
    _require(vmi.device == occ.device and intr.device == occ.device, "occ, vmi and intr must be on one device")
    B, dimz, dimy, dimx = (int(v) for v in occ.shape)
    vmi = vmi.contiguous().reshape(-1)
    intr = intr.contiguous()
    _require(vmi.numel() % (16 * B) == 0 and vmi.numel() > 0, "vmi must hold B*V*16 floats")
    _require(intr.numel() == 4 * B, "intr must be [B,4]")
    V = vmi.numel() // (16 * B)
    H, W, n_rows = int(H), int(W), int(n_rows)
    dev = occ.device
    ws = workspace if workspace is not None else get_workspace(dev)
    ptr = ws.ensure(workspace_bytes(B, V, H, W, 1, dimz, dimy, dimx, n_rows), dev)
    key = (occ._version, occ.data_ptr(), tuple(occ.shape), n_rows)
    prev = ws.accel_key
    reuse = prev is not None and prev[0]() is occ and prev[1] == key and ACCEL_CACHE
    if exact_march is None:
        exact_march = EXACT_MARCH
    flags = VP_FLAG_SYNC | (VP_FLAG_REUSE_ACCEL if reuse else 0) | (VP_FLAG_EXACT_MARCH if exact_march else 0)
    ids = torch.empty((B, V, H, W), dtype=torch.int32, device=dev)
    o = (ctypes.c_float * 5)(*[float(v) for v in opts5])
    g = (ctypes.c_float * 3)(*[float(v) for v in grid_origin3])
    with torch.cuda.device(dev):
        rc = lib().vp_first_hit_ids(occ.data_ptr(), vmi.data_ptr(), intr.data_ptr(), o, g, ctypes.c_float(float(voxel_size)),
                                    B, V, H, W, dimz, dimy, dimx, n_rows, ids.data_ptr(), ptr, ws.capacity(),
                                    torch.cuda.current_stream(dev).cuda_stream, flags)
    if rc != VP_OK:
        ws.accel_key = None
        check(rc)
    ws.accel_key = (weakref.ref(occ), key)
    return ids


def render_features(ids, rows, dtype=None, out=None, check=True):
    """vp_render_features: out[..., :] = rows[ids[...], :] -- every pixel takes the row of its first-hit voxel; zeros where
    the ID is 0 (a miss) or outside [0, n_rows).  ids int32 CUDA (e.g. [B,V,H,W] from first_hit_ids), rows float32 [n_rows, C]
    on the same device; returns ids.shape + (C,) in ``dtype`` (float32 or float16, rounded to nearest-even), or fills ``out``.
    Asynchronous on the current stream, except with ``check``: then the out-of-range IDs are counted, the call synchronises and
    raises VoxprojError if there were any.  The adjoint of the forward projection (project_features_autograd uses it)."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    _require(dtype in (torch.float32, torch.float16), f"dtype must be torch.float32 or torch.float16, not {dtype}")
    _require_tensors((ids, "ids", (torch.int32,)), (rows, "rows", (torch.float32,)))
    _require(rows.dim() == 2 and rows.shape[0] > 0 and rows.shape[1] > 0, "rows must be [n_rows, C] with n_rows, C >= 1")
    _require(rows.device == ids.device, "ids and rows must be on one device")
    _require(ids.numel() > 0, "ids is empty")
    ids = ids.contiguous()
    rows = rows.contiguous()
    n_rows, C = (int(v) for v in rows.shape)
    shape = tuple(ids.shape) + (C,)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=ids.device)
    _require(isinstance(out, torch.Tensor) and out.is_cuda and out.device == ids.device and out.dtype == dtype
             and tuple(out.shape) == shape and out.is_contiguous(), f"out must be a contiguous {dtype} CUDA tensor of shape {shape}")
    bad = torch.zeros(1, dtype=torch.int32, device=ids.device) if check else None
    _call(ids.device, "vp_render_features", ids.data_ptr(), ids.numel(), rows.data_ptr(), n_rows, C, out.data_ptr(),
          int(dtype == torch.float16), _ptr(bad))
    if check:
        n_bad = int(bad.item())
        if n_bad:
            raise VoxprojError(f"render_features: {n_bad} pixel(s) carry an ID outside [0, {n_rows}) (rendered as zeros)")
    return out


def query_features(rows, text, scale=1.0, want_logits=True, want_margin=True, check=True):
    """vp_query_features: score every row of a feature table against P text embeddings.  rows float16 or float32 CUDA [N, C]
    (any row stride, unit channel stride), text [P, C] (any float dtype; used as float32) on the same device, scale > 0 the
    logit multiplier (1.0: cosine similarity; LSeg's head multiplies by its logit_scale).  Returns (labels int32 [N],
    logits float32 [N, P] or None, margin float32 [N] or None) on the rows' device: label = argmax of
    scale * cos(row, text_j) (lowest index on ties), margin = softmax top-1 minus top-2 (1 when P = 1).  A row with a
    non-finite element gets label -1 and NaN logits / margin.  Asynchronous on the current stream, except with ``check``: then
    the call synchronises and raises VoxprojError if any row was non-finite."""
    import torch
    _require_tensors((rows, "rows", (torch.float16, torch.float32)),
                     (text, "text", (torch.float16, torch.bfloat16, torch.float32, torch.float64)))
    _require(rows.dim() == 2 and rows.shape[1] > 0, "rows must be [N, C] with C >= 1")
    _require(text.dim() == 2 and text.shape[0] > 0, "text must be [P, C] with P >= 1")
    _require(rows.device == text.device, "rows and text must be on one device")
    N, C = (int(v) for v in rows.shape)
    P = int(text.shape[0])
    _require(int(text.shape[1]) == C, f"text has {int(text.shape[1])} channels, rows have {C}")
    _require(1 <= P <= 1024 and C <= 2048, f"P = {P} must be in [1, 1024] and C = {C} in [1, 2048]")
    scale = float(scale)
    _require(scale > 0 and scale != float("inf"), f"scale must be finite and > 0, not {scale}")
    dev = rows.device
    if rows.stride(1) != 1 or rows.stride(0) < C:
        rows = rows.contiguous()
    text = text.to(torch.float32).contiguous()
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    logits = torch.empty((N, P), dtype=torch.float32, device=dev) if want_logits else None
    margin = torch.empty(N, dtype=torch.float32, device=dev) if want_margin else None
    if N == 0:
        return labels, logits, margin
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if check else None
    nbytes = int(_entry("vp_query_workspace_bytes")(P, C))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    ws_ptr = (ws.data_ptr() + 255) & ~255
    _call(dev, "vp_query_features", rows.data_ptr(), int(rows.dtype == torch.float16), N, C, int(rows.stride(0)),
          text.data_ptr(), P, scale, _ptr(logits), labels.data_ptr(), _ptr(margin), _ptr(bad), ws_ptr, nbytes)
    if check:
        n_bad = int(bad.item())
        if n_bad:
            raise VoxprojError(f"query_features: {n_bad} row(s) hold a non-finite element (label -1, NaN logits)")
    return labels, logits, margin


SplatResult = collections.namedtuple("SplatResult", "labels confidence alpha logits n_isect n_nonfinite")


class SplatWorkspace:
    """Grow-only device scratch of the Gaussian splatting calls (vp_splat_*), allocated through torch's allocator.  Unlike
    Workspace it is not announced to the library: the splatting calls keep no state with the buffer."""

    def __init__(self):
        self.buf = None

    def ensure(self, nbytes, device, keep=0):
        """A 256-byte aligned pointer to at least ``nbytes``; when the buffer grows, its first ``keep`` bytes are copied."""
        import torch
        if self.buf is None or self.buf.device != device or self.capacity() < nbytes:
            old = self.buf
            self.buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
            if keep and old is not None and old.device == device:
                o = (old.data_ptr() + 255) & ~255
                self.buf[self.ptr() - self.buf.data_ptr():][:keep].copy_(old[o - old.data_ptr():][:keep])
        return self.ptr()

    def ptr(self):
        return (self.buf.data_ptr() + 255) & ~255

    def capacity(self):
        return 0 if self.buf is None else self.buf.numel() - (self.ptr() - self.buf.data_ptr())


def _splat_camera(viewmat, K, W, H):
    import torch
    vm = torch.as_tensor(viewmat, dtype=torch.float64).detach().cpu().reshape(-1)
    k = torch.as_tensor(K, dtype=torch.float64).detach().cpu()
    _require(vm.numel() == 16, "viewmat must be a [4, 4] world-to-camera matrix")
    _require(tuple(k.shape) == (3, 3), "K must be [3, 3]")
    _require(1 <= int(W) <= 32768 and 1 <= int(H) <= 32768, f"image size {W} x {H} outside [1, 32768]")
    return (ctypes.c_float * 16)(*vm.tolist()), [float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])]


def _splat_gaussians(means, quats, scales, opacities=None, dev=None):
    """The N x 3 / 4 / 3 (and N) float32 Gaussian tensors on one GPU (``dev``, default the means'): N and contiguous tensors."""
    import torch
    named = [(means, "means"), (quats, "quats"), (scales, "scales")] + ([(opacities, "opacities")] if opacities is not None else [])
    _require_tensors(*((t, name, (torch.float32,)) for t, name in named))
    N = int(means.shape[0]) if means.dim() == 2 else -1
    _require(tuple(means.shape) == (N, 3) and N >= 0, "means must be [N, 3]")
    _require(tuple(quats.shape) == (N, 4), f"quats must be [{N}, 4]")
    _require(tuple(scales.shape) == (N, 3), f"scales must be [{N}, 3]")
    _require(opacities is None or tuple(opacities.shape) == (N,), f"opacities must be [{N}]")
    dev = means.device if dev is None else dev
    _require(all(t.device == dev for t, _ in named), "the Gaussian tensors must be on one device")
    return N, [t.contiguous() for t, _ in named]


def _splat_rows(features, n=None):
    """The float32 feature rows [n, D] (any row count when ``n`` is None), 1 <= D <= 64, with a unit channel stride and a
    row stride >= D (a contiguous copy otherwise): (features, D)."""
    import torch
    _require_tensors((features, "features", (torch.float32,)))
    _require(features.dim() == 2 and (n is None or int(features.shape[0]) == int(n)),
             f"features must be [{'N' if n is None else n}, D]")
    D = int(features.shape[1])
    _require(1 <= D <= 64, f"D = {D} outside [1, 64]")
    if features.stride(1) != 1 or features.stride(0) < D:
        features = features.contiguous()
    return features, D


def _splat_images(dev, *specs):
    """(tensor or None, name, shape, dtype) per optional image on the features' device ``dev`` (shape None: one element):
    the contiguous tensors, None kept."""
    out = []
    for t, name, shape, dtype in specs:
        if t is not None:
            _require_tensors((t, name, (dtype,)))
            _require(t.device == dev and (t.numel() == 1 if shape is None else tuple(t.shape) == tuple(int(v) for v in shape)),
                     f"{name} must be {'one element' if shape is None else list(shape)} on the features' device")
            t = t.contiguous()
        out.append(t)
    return out


def _splat_workspace_bytes(n_gaussians, W, H, capacity):
    """vp_splat_workspace_bytes for ``capacity`` intersections; a size of 0 (an argument out of range) is refused."""
    nbytes = int(lib().vp_splat_workspace_bytes(int(n_gaussians), int(W), int(H), int(capacity)))
    _require(nbytes > 0, f"no workspace size for N = {n_gaussians}, {W} x {H}, capacity {capacity}")
    return nbytes


def _splat_forward_workspace(workspace, n_gaussians, W, H, capacity, dev, size=_splat_workspace_bytes):
    """Grow the projection's workspace to ``capacity`` intersections (the projection's bytes kept): its pointer.  ``size``:
    the family's size function (the mesh rasterizer passes its own)."""
    need = size(n_gaussians, W, H, capacity)
    return workspace.ensure(need, dev, keep=size(n_gaussians, W, H, 0))


def _filled_workspace(caller, forward, workspace, need, dev):
    """Check that ``workspace`` can be the one a ``forward`` call filled (on ``dev``, at least ``need`` bytes): its pointer."""
    _require(workspace is not None and workspace.buf is not None and workspace.buf.device == dev and
             workspace.capacity() >= need, f"{caller} needs the workspace of a {forward} call")
    return workspace.ptr()


def _splat_backward_workspaces(caller, forward, workspace, bwd_workspace, n_gaussians, W, H, capacity, D, geom, dev):
    """Check that ``workspace`` is the one a ``forward`` call left, and size the backward scratch (rows with the five
    screen sums when ``geom``): (the scratch's SplatWorkspace, its pointer)."""
    _filled_workspace(caller, forward, workspace, _splat_workspace_bytes(n_gaussians, W, H, capacity), dev)
    L = lib()
    need = int((L.vp_splat_geometry_backward_workspace_bytes if geom else L.vp_splat_backward_workspace_bytes)(int(capacity), D))
    _require(need > 0, f"no backward workspace size for capacity {capacity}, D = {D}")
    bw = bwd_workspace if bwd_workspace is not None else SplatWorkspace()
    return bw, bw.ensure(need, dev)


def _splat_grads(N, D, dev, **want):
    """The dict of the backward calls' outputs: an empty float32 tensor per gradient asked for, None for the others."""
    import torch
    tails = {"means": (3,), "quats": (4,), "scales": (3,), "features": (D,), "opacities": (), "screen": (5,)}
    return {name: torch.empty((N,) + tail, dtype=torch.float32, device=dev) if want.get(name) else None
            for name, tail in tails.items()}


def _ptr(t):
    """The device pointer of an optional tensor: NULL for None and for an empty tensor."""
    return t.data_ptr() if t is not None and t.numel() else None


def splat_project(means, quats, scales, opacities, viewmat, K, W, H, *, near=0.01, far=1e10, eps2d=0.3, workspace=None,
                  n_nonfinite=None):
    """vp_splat_project: screen-space records of every Gaussian into ``workspace`` (a SplatWorkspace; grown to the
    projection's size).  Returns the device int64 [1] intersection count (not read here).  ``n_nonfinite``: optional device
    int32 [1] that counts the Gaussians culled for a non-finite parameter."""
    import torch
    N, (means, quats, scales, opacities) = _splat_gaussians(means, quats, scales, opacities)
    dev = means.device
    vm, (fx, fy, cx, cy) = _splat_camera(viewmat, K, W, H)
    ws = workspace if workspace is not None else SplatWorkspace()
    nbytes = int(lib().vp_splat_workspace_bytes(N, int(W), int(H), 0))
    _require(nbytes > 0, f"no workspace size for N = {N}, {W} x {H}")
    ptr = ws.ensure(nbytes, dev)
    n_isect = torch.zeros(1, dtype=torch.int64, device=dev)
    _call(dev, "vp_splat_project", means.data_ptr(), quats.data_ptr(), scales.data_ptr(), opacities.data_ptr(), N, vm,
          fx, fy, cx, cy, int(W), int(H), float(near), float(far), float(eps2d), n_isect.data_ptr(),
          n_nonfinite.data_ptr() if n_nonfinite is not None else None, ptr, ws.capacity())
    return n_isect


def splat_rasterize(features, n_gaussians, W, H, capacity, workspace, *, want_logits=False, want_alpha=False,
                    want_confidence=True, status=None):
    """vp_splat_rasterize after splat_project on ``workspace``: sort ``capacity`` intersection keys, blend, epilogue.  The
    workspace grows to ``capacity`` (the projection's bytes kept).  Returns (labels int32 [H,W], confidence f32 [H,W] or None,
    alpha f32 [H,W] or None, logits f32 [D,H,W] or None).  ``status``: optional device int32 [1], set to 1 when the device
    count exceeds ``capacity`` (then no output is written)."""
    import torch
    features, D = _splat_rows(features, n_gaussians)
    dev = features.device
    ptr = _splat_forward_workspace(workspace, n_gaussians, W, H, capacity, dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    conf = torch.empty((H, W), dtype=torch.float32, device=dev) if want_confidence else None
    alpha = torch.empty((H, W), dtype=torch.float32, device=dev) if want_alpha else None
    logits = torch.empty((D, H, W), dtype=torch.float32, device=dev) if want_logits else None
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _call(dev, "vp_splat_rasterize", features.data_ptr(), D, max(int(features.stride(0)), D), int(n_gaussians), int(W),
          int(H), int(capacity), labels.data_ptr(), p(conf), p(alpha), p(logits), p(status), ptr, workspace.capacity())
    return labels, conf, alpha, logits


def splat_rasterize_backward(features, n_gaussians, W, H, capacity, workspace, grad_logits=None, grad_alpha=None, *,
                             bwd_workspace=None, want_features=True, want_opacities=True, status=None):
    """vp_splat_rasterize_backward after splat_rasterize on ``workspace`` with the same features, n_gaussians, W, H and
    capacity: gradients of sum(grad_logits * logits) + sum(grad_alpha * alpha) with respect to the features and the
    activated opacities.  grad_logits f32 [D,H,W] and grad_alpha f32 [H,W] on the features' GPU, each may be None (zero).
    ``bwd_workspace``: a SplatWorkspace for the per-intersection partials (a fresh one when None).  Returns (grad_features
    f32 [N,D] or None, grad_opacities f32 [N] or None).  ``status``: optional device int32 [1], set to 1 when the device count
    exceeds ``capacity`` (then nothing is written)."""
    import torch
    features, D = _splat_rows(features, n_gaussians)
    dev, N = features.device, int(n_gaussians)
    grad_logits, grad_alpha = _splat_images(dev, (grad_logits, "grad_logits", (D, H, W), torch.float32),
                                            (grad_alpha, "grad_alpha", (H, W), torch.float32))
    bw, bptr = _splat_backward_workspaces("splat_rasterize_backward", "splat_rasterize", workspace, bwd_workspace, N, W, H,
                                          capacity, D, False, dev)
    out = _splat_grads(N, D, dev, features=want_features, opacities=want_opacities)
    _call(dev, "vp_splat_rasterize_backward", _ptr(features), D, max(int(features.stride(0)), D), N, int(W), int(H),
          int(capacity), _ptr(grad_logits), _ptr(grad_alpha), _ptr(out["features"]), _ptr(out["opacities"]), _ptr(status),
          workspace.ptr(), workspace.capacity(), bptr, bw.capacity())
    return out["features"], out["opacities"]


def splat_rasterize_backward_geometry(means, quats, scales, features, viewmat, K, W, H, capacity, workspace, grad_logits=None,
                                      grad_alpha=None, *, eps2d=0.3, bwd_workspace=None, want_means=True, want_quats=True,
                                      want_scales=True, want_features=True, want_opacities=True, want_screen=False,
                                      status=None):
    """vp_splat_rasterize_backward_geometry after splat_rasterize on ``workspace``: one fused call for the gradients of
    sum(grad_logits * logits) + sum(grad_alpha * alpha) with respect to the means, the quaternions (as passed), the activated
    scales, the features and the activated opacities, plus the five screen-space sums per Gaussian (dL/d mean2d, dL/d conic)
    when ``want_screen``.  means, quats, scales, viewmat, K and eps2d are those of the splat_project call; the rest is as
    splat_rasterize_backward, whose grad_features / grad_opacities this call reproduces bit for bit.  ``bwd_workspace``: a
    SplatWorkspace of vp_splat_geometry_backward_workspace_bytes (a fresh one when None).  Returns a dict with the keys
    means [N,3], quats [N,4], scales [N,3], features [N,D], opacities [N], screen [N,5]; None for what was not asked."""
    import torch
    _require_tensors(*((t, name, (torch.float32,)) for t, name in
                       ((means, "means"), (quats, "quats"), (scales, "scales"), (features, "features"))))
    N, (means, quats, scales) = _splat_gaussians(means, quats, scales, dev=features.device)
    features, D = _splat_rows(features, N)
    dev = features.device
    grad_logits, grad_alpha = _splat_images(dev, (grad_logits, "grad_logits", (D, H, W), torch.float32),
                                            (grad_alpha, "grad_alpha", (H, W), torch.float32))
    vm, (fx, fy, cx, cy) = _splat_camera(viewmat, K, W, H)
    bw, bptr = _splat_backward_workspaces("splat_rasterize_backward_geometry", "splat_rasterize", workspace, bwd_workspace, N,
                                          W, H, capacity, D, True, dev)
    out = _splat_grads(N, D, dev, means=want_means, quats=want_quats, scales=want_scales, features=want_features,
                       opacities=want_opacities, screen=want_screen)
    _call(dev, "vp_splat_rasterize_backward_geometry", _ptr(means), _ptr(quats), _ptr(scales), _ptr(features), D,
          max(int(features.stride(0)), D), N, vm, fx, fy, cx, cy, int(W), int(H), float(eps2d), int(capacity),
          _ptr(grad_logits), _ptr(grad_alpha), _ptr(out["means"]), _ptr(out["quats"]), _ptr(out["scales"]),
          _ptr(out["features"]), _ptr(out["opacities"]), _ptr(out["screen"]), _ptr(status), workspace.ptr(),
          workspace.capacity(), bptr, bw.capacity())
    return out


def _splat_sized_view(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, workspace):
    """splat_project, then the one read of the 8-byte intersection count that sizes the sort: (workspace, capacity, the
    device counter of non-finite Gaussians, the device status word for the rasterize call)."""
    import torch
    ws = workspace if workspace is not None else SplatWorkspace()
    bad = torch.zeros(1, dtype=torch.int32, device=means.device)
    status = torch.zeros(1, dtype=torch.int32, device=means.device)
    n_isect = splat_project(means, quats, scales, opacities, viewmat, K, W, H, near=near, far=far, eps2d=eps2d,
                            workspace=ws, n_nonfinite=bad)
    cap = int(n_isect.item())
    _require(cap <= 2 ** 31 - 1, f"{cap} tile intersections: more than 2^31 - 1")
    return ws, cap, bad, status


def _splat_view_check(caller, status, bad, unwritten):
    """Read the status word and the non-finite counter (one synchronisation) and raise VoxprojError on either."""
    import torch
    st, n_bad = (int(v) for v in torch.cat([status, bad]).tolist())
    if st:
        raise VoxprojError(f"{caller}: the intersection count outgrew the workspace ({unwritten})")
    if n_bad:
        raise VoxprojError(f"{caller}: {n_bad} Gaussian(s) have a non-finite parameter (culled)")


def splat_features(means, quats, scales, opacities, features, viewmat, K, W, H, *, want_logits=False, want_alpha=False,
                   want_confidence=True, near=0.01, far=1e10, eps2d=0.3, workspace=None, check=True):
    """Splat D-channel per-Gaussian features into one W x H view (vp_splat_project + vp_splat_rasterize; the contract is in
    include/voxproj.h).  means f32 [N,3], quats f32 [N,4] (w, x, y, z; normalised here), scales f32 [N,3] and opacities f32
    [N] (both activated), features f32 [N,D] (D <= 64, any row stride), all on one GPU; viewmat [4,4] world-to-camera and K
    [3,3] (any device; read on the host).  Reads the 8-byte intersection count once to size the workspace (a SplatWorkspace,
    kept and regrown across calls when given).  Returns SplatResult(labels int32 [H,W], confidence f32 [H,W] or None, alpha
    f32 [H,W] or None, logits f32 [D,H,W] or None, n_isect int, n_nonfinite device int32 [1]).  With ``check`` the call
    synchronises once more and raises VoxprojError when a Gaussian had a non-finite parameter (it is culled)."""
    import torch
    for t, name in ((means, "means"), (quats, "quats"), (scales, "scales"), (opacities, "opacities"), (features, "features")):
        _require(isinstance(t, torch.Tensor) and t.dtype == torch.float32, f"{name} must be a torch.float32 tensor")
    _require(features.dim() == 2 and features.shape[0] == means.shape[0],
             "features must be [N, D] with one row per Gaussian")
    _require(1 <= int(features.shape[1]) <= 64, f"D = {int(features.shape[1])} outside [1, 64]")
    _require_tensors(*((t, name, (torch.float32,)) for t, name in
                       ((means, "means"), (quats, "quats"), (scales, "scales"), (opacities, "opacities"), (features, "features"))))
    _require(features.device == means.device, "features and the Gaussians must be on one device")
    ws, cap, bad, status = _splat_sized_view(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, workspace)
    labels, conf, alpha, logits = splat_rasterize(features, int(means.shape[0]), W, H, cap, ws, want_logits=want_logits,
                                                  want_alpha=want_alpha, want_confidence=want_confidence, status=status)
    if check:
        _splat_view_check("splat_features", status, bad, "no image written")
    return SplatResult(labels, conf, alpha, logits, cap, bad)


SplatLossResult = collections.namedtuple("SplatLossResult",
                                         "loss_stats pixel_loss labels confidence alpha logits n_isect n_nonfinite")
_REDUCTIONS = {"sum": VP_LOSS_SUM, "mean": VP_LOSS_MEAN}


def _splat_loss_maps(target, pixel_weight, W, H, dev):
    import torch
    _require_tensors((target, "target", (torch.int32,)))
    _require(tuple(target.shape) == (int(H), int(W)) and target.device == dev, f"target must be int32 [{H}, {W}] on the features' device")
    if pixel_weight is not None:
        _require_tensors((pixel_weight, "pixel_weight", (torch.float32,)))
        _require(tuple(pixel_weight.shape) == (int(H), int(W)) and pixel_weight.device == dev,
                 f"pixel_weight must be float32 [{H}, {W}] on the features' device")
        pixel_weight = pixel_weight.contiguous()
    return target.contiguous(), pixel_weight


def splat_rasterize_loss(features, n_gaussians, W, H, capacity, workspace, target, pixel_weight=None, *, want_pixel_loss=False,
                         want_labels=True, want_confidence=True, want_alpha=False, want_logits=False, loss_workspace=None,
                         status=None):
    """vp_splat_rasterize_loss after splat_project on ``workspace``: splat_rasterize with the fused softmax cross-entropy
    epilogue.  target int32 [H,W] (valid when 0 <= target < D, anything else ignored), pixel_weight f32 [H,W] or None (1).
    Returns (loss_stats f64 [2] = {sum w l, sum w} on the device, pixel_loss f32 [H,W] or None, labels, confidence, alpha,
    logits as splat_rasterize, each None unless asked for).  ``loss_workspace``: a SplatWorkspace for the per-tile sums (a
    fresh one when None)."""
    import torch
    features, D = _splat_rows(features, n_gaussians)
    dev = features.device
    target, pixel_weight = _splat_loss_maps(target, pixel_weight, W, H, dev)
    ptr = _splat_forward_workspace(workspace, n_gaussians, W, H, capacity, dev)
    lw = loss_workspace if loss_workspace is not None else SplatWorkspace()
    lptr = lw.ensure(int(lib().vp_splat_loss_workspace_bytes(int(W), int(H))), dev)
    img = lambda want, dtype, *lead: torch.empty(lead + (H, W), dtype=dtype, device=dev) if want else None  # noqa: E731
    stats = torch.zeros(2, dtype=torch.float64, device=dev)
    ploss = img(want_pixel_loss, torch.float32)
    labels, conf = img(want_labels, torch.int32), img(want_confidence, torch.float32)
    alpha, logits = img(want_alpha, torch.float32), img(want_logits, torch.float32, D)
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _call(dev, "vp_splat_rasterize_loss", _ptr(features), D, max(int(features.stride(0)), D), int(n_gaussians), int(W),
          int(H), int(capacity), p(target), p(pixel_weight), p(stats), p(ploss), p(labels), p(conf), p(alpha), p(logits),
          p(status), ptr, workspace.capacity(), lptr, lw.capacity())
    return stats, ploss, labels, conf, alpha, logits


def splat_loss_backward(means, quats, scales, features, viewmat, K, W, H, capacity, workspace, target, pixel_weight=None,
                        loss_stats=None, *, logits=None, reduction="mean", grad_loss=None, grad_alpha=None, eps2d=0.3,
                        bwd_workspace=None, want_means=False, want_quats=False, want_scales=False, want_features=True,
                        want_opacities=True, want_screen=False, status=None):
    """vp_splat_loss_backward after splat_rasterize_loss on ``workspace``: the gradients of the (sum or mean) cross-entropy,
    scaled by ``grad_loss`` (device f32 [1], None = 1), plus sum(grad_alpha * alpha).  ``logits``: the image the forward
    wrote (the saved arm) or None (the replay arm: the sweep blends each pixel again); both give the same bits.
    ``loss_stats``: the forward's, read on the device for the mean.  Without a geometry or screen gradient the call runs the
    sweep of splat_rasterize_backward (means, quats, scales, viewmat and K may then be None), otherwise the geometry
    sweep.  Returns the dict of splat_rasterize_backward_geometry."""
    import torch
    _require(reduction in _REDUCTIONS, f"reduction must be 'sum' or 'mean', not {reduction!r}")
    features, D = _splat_rows(features)
    N, dev = int(features.shape[0]), features.device
    chain = want_means or want_quats or want_scales
    geom = chain or want_screen
    vm, fx, fy, cx, cy = None, 1.0, 1.0, 0.0, 0.0
    if chain:
        _require_tensors(*((t, name, (torch.float32,)) for t, name in ((means, "means"), (quats, "quats"), (scales, "scales"))))
        _require(tuple(means.shape) == (N, 3) and tuple(quats.shape) == (N, 4) and tuple(scales.shape) == (N, 3),
                 f"means, quats, scales must be [{N}, 3], [{N}, 4], [{N}, 3]")
        _, (means, quats, scales) = _splat_gaussians(means, quats, scales, dev=dev)
        vm, (fx, fy, cx, cy) = _splat_camera(viewmat, K, W, H)
    else:
        means = quats = scales = None
    target, pixel_weight = _splat_loss_maps(target, pixel_weight, W, H, dev)
    logits, grad_alpha, grad_loss, loss_stats = _splat_images(
        dev, (logits, "logits", (D, H, W), torch.float32), (grad_alpha, "grad_alpha", (H, W), torch.float32),
        (grad_loss, "grad_loss", None, torch.float32), (loss_stats, "loss_stats", (2,), torch.float64))
    _require(loss_stats is not None, "loss_stats (the forward's) is required")
    bw, bptr = _splat_backward_workspaces("splat_loss_backward", "splat_rasterize_loss", workspace, bwd_workspace, N, W, H,
                                          capacity, D, geom, dev)
    out = _splat_grads(N, D, dev, means=want_means, quats=want_quats, scales=want_scales, features=want_features,
                       opacities=want_opacities, screen=want_screen)
    _call(dev, "vp_splat_loss_backward", _ptr(means), _ptr(quats), _ptr(scales), _ptr(features), D,
          max(int(features.stride(0)), D), N, vm, fx, fy, cx, cy, int(W), int(H), float(eps2d), int(capacity), _ptr(target),
          _ptr(pixel_weight), _ptr(logits), _ptr(loss_stats), _REDUCTIONS[reduction], _ptr(grad_loss), _ptr(grad_alpha),
          _ptr(out["means"]), _ptr(out["quats"]), _ptr(out["scales"]), _ptr(out["features"]), _ptr(out["opacities"]),
          _ptr(out["screen"]), _ptr(status), workspace.ptr(), workspace.capacity(), bptr, bw.capacity())
    return out


def splat_loss(means, quats, scales, opacities, features, viewmat, K, W, H, target, pixel_weight=None, *,
               want_pixel_loss=False, want_labels=True, want_confidence=True, want_alpha=False, want_logits=False, near=0.01,
               far=1e10, eps2d=0.3, workspace=None, loss_workspace=None, check=True):
    """Splat the features into one view and take the fused cross-entropy against ``target`` (vp_splat_project +
    vp_splat_rasterize_loss), as splat_features splats: reads the 8-byte intersection count once to size the sort.
    Returns SplatLossResult(loss_stats f64 [2] on the device = {sum w l, sum w}, pixel_loss, labels, confidence, alpha,
    logits, n_isect int, n_nonfinite device int32 [1])."""
    import torch
    _require_tensors(*((t, name, (torch.float32,)) for t, name in
                       ((means, "means"), (quats, "quats"), (scales, "scales"), (opacities, "opacities"), (features, "features"))))
    _require(features.dim() == 2 and features.shape[0] == means.shape[0], "features must be [N, D] with one row per Gaussian")
    _require(features.device == means.device, "features and the Gaussians must be on one device")
    ws, cap, bad, status = _splat_sized_view(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, workspace)
    out = splat_rasterize_loss(features, int(means.shape[0]), W, H, cap, ws, target, pixel_weight,
                               want_pixel_loss=want_pixel_loss, want_labels=want_labels, want_confidence=want_confidence,
                               want_alpha=want_alpha, want_logits=want_logits, loss_workspace=loss_workspace, status=status)
    if check:
        _splat_view_check("splat_loss", status, bad, "nothing written")
    return SplatLossResult(*out, cap, bad)


def splat_lift_workspace_bytes(capacity, C):
    """vp_splat_lift_workspace_bytes: bytes of the lift's scratch for ``capacity`` intersections and C channels (0 when
    either is out of range).  Needs no GPU."""
    return int(_entry("vp_splat_lift_workspace_bytes")(int(capacity), int(C)))


def splat_lift(feats, n_gaussians, W, H, capacity, workspace, sum, wsum, pixel_weight=None, sorted=False, status=None,
               lift_workspace=None):
    """vp_splat_lift after splat_project on ``workspace``: add one view's blend-weighted feature sums to the Gaussians.
    feats f16 [H,W,C] channels-last (unit channel stride, any pixel stride >= C; what upsample_features(keep_dtype=True)
    returns), sum f32 [N,C] (unit channel stride) and wsum f32 [N] or None, all on one GPU; both accumulate and are never
    cleared.  pixel_weight f32 [H,W] or None (1).  ``sorted``: False sorts ``capacity`` keys first (valid directly after
    splat_project; the workspace grows as for splat_rasterize), True reuses the sort a splat_rasterize / splat_rasterize_loss
    call with the same capacity left.  ``lift_workspace``: a SplatWorkspace for the partial rows (a fresh one when None).
    ``status``: optional device int32 [1], set to 1 when the device count exceeds ``capacity`` (then nothing is added)."""
    import torch
    _require(isinstance(sorted, (bool, int)) and int(sorted) in (0, 1), "sorted must be False or True")
    _require_tensors((feats, "feats", (torch.float16,)), (sum, "sum", (torch.float32,)))
    dev, N = feats.device, int(n_gaussians)
    _require(feats.dim() == 3 and tuple(feats.shape[:2]) == (int(H), int(W)), f"feats must be [{H}, {W}, C]")
    C = int(feats.shape[2])
    _require(1 <= C <= 4096, f"C = {C} outside [1, 4096]")
    if feats.stride(2) != 1 or feats.stride(1) < C or feats.stride(0) != int(W) * feats.stride(1):
        feats = feats.contiguous()
    _require(sum.dim() == 2 and tuple(sum.shape) == (N, C) and sum.device == dev and (N == 0 or sum.stride(1) == 1) and
             (N <= 1 or sum.stride(0) >= C), f"sum must be float32 [{N}, {C}] with a unit channel stride on the map's device")
    if wsum is not None:
        _require_tensors((wsum, "wsum", (torch.float32,)))
        _require(tuple(wsum.shape) == (N,) and wsum.device == dev and wsum.is_contiguous(),
                 f"wsum must be contiguous float32 [{N}] on the map's device")
    (pixel_weight,) = _splat_images(dev, (pixel_weight, "pixel_weight", (H, W), torch.float32))
    if sorted:
        ptr = _filled_workspace("splat_lift(sorted=True)", "splat_rasterize", workspace,
                                _splat_workspace_bytes(N, W, H, capacity), dev)
    else:
        ptr = _splat_forward_workspace(workspace, N, W, H, capacity, dev)
    need = splat_lift_workspace_bytes(capacity, C)
    _require(need > 0, f"no lift workspace size for capacity {capacity}, C = {C}")
    lw = lift_workspace if lift_workspace is not None else SplatWorkspace()
    lptr = lw.ensure(need, dev)
    _call(dev, "vp_splat_lift", feats.data_ptr(), C, int(feats.stride(1)), _ptr(pixel_weight), N, int(W), int(H),
          int(capacity), int(sorted), sum.data_ptr() if N else lptr, max(int(sum.stride(0)), C) if N else C, _ptr(wsum),
          _ptr(status), ptr, workspace.capacity(), lptr, lw.capacity())


def splat_lift_view(means, quats, scales, opacities, feats, viewmat, K, W, H, sum, wsum, pixel_weight=None, *, near=0.01,
                    far=1e10, eps2d=0.3, workspace=None, lift_workspace=None, check=True):
    """Lift one view's fp16 feature map onto the Gaussians (vp_splat_project + vp_splat_lift), as splat_features splats:
    reads the 8-byte intersection count once to size the sort and the scratch.  ``sum`` / ``wsum`` accumulate.  Returns
    (n_isect int, n_nonfinite device int32 [1]).  With ``check`` the call synchronises once more and raises VoxprojError when
    a Gaussian had a non-finite parameter (it is culled)."""
    import torch
    _require_tensors(*((t, name, (torch.float32,)) for t, name in
                       ((means, "means"), (quats, "quats"), (scales, "scales"), (opacities, "opacities"))))
    _require(isinstance(feats, torch.Tensor) and feats.device == means.device, "feats and the Gaussians must be on one device")
    ws, cap, bad, status = _splat_sized_view(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, workspace)
    splat_lift(feats, int(means.shape[0]), W, H, cap, ws, sum, wsum, pixel_weight, sorted=False, status=status,
               lift_workspace=lift_workspace)
    if check:
        _splat_view_check("splat_lift_view", status, bad, "nothing added")
    return cap, bad


class GaussianFeatureLifter:
    """Blend-weighted mean of the pixel features every Gaussian contributed to, over any number of views:
    F_g = sum_views sum_p m_p w_g(p) feat_v(p) / sum_views sum_p m_p w_g(p).  ``add_view`` accumulates one view's sums
    (splat_lift_view), ``finish`` divides."""

    def __init__(self, n, C, device):
        import torch
        self.n, self.C, self.device = int(n), int(C), torch.device(device)
        self.sum = torch.zeros((self.n, self.C), dtype=torch.float32, device=self.device)
        self.wsum = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.views = 0
        self._ws = self._lw = None
        if self.device.type == "cuda":
            self._ws, self._lw = SplatWorkspace(), SplatWorkspace()

    def add_view(self, means, quats, scales, opacities, feats, viewmat, K, W, H, pixel_weight=None, **kw):
        """One view's map f16 [H,W,C] into the sums; returns splat_lift_view's (n_isect, n_nonfinite)."""
        _require(int(means.shape[0]) == self.n and int(feats.shape[-1]) == self.C,
                 f"add_view needs {self.n} Gaussians and a map of {self.C} channels")
        out = splat_lift_view(means, quats, scales, opacities, feats, viewmat, K, W, H, self.sum, self.wsum, pixel_weight,
                              workspace=self._ws, lift_workspace=self._lw, **kw)
        self.views += 1
        return out

    def finish(self, min_weight=1e-3):
        """(avg_feats f16 [n,C], weight f32 [n], valid bool [n]): sum / weight where weight >= min_weight (and > 0), rows of
        zeros elsewhere."""
        import torch
        valid = (self.wsum >= float(min_weight)) & (self.wsum > 0)
        avg = torch.where(valid[:, None], self.sum / self.wsum.clamp_min(torch.finfo(torch.float32).tiny)[:, None],
                          torch.zeros((), dtype=torch.float32, device=self.device))
        return avg.to(torch.float16), self.wsum.clone(), valid


def splat_render(rows, n_gaussians, W, H, capacity, workspace, *, out=None, dtype=None, want_alpha=False, sorted=False,
                 status=None, check=True):
    """vp_splat_render after splat_project on ``workspace``: blend the Gaussians' wide rows into one view,
    out[y, x, c] = sum_g w_g(p) rows[g, c], with the weights vp_splat_rasterize blends with.  rows f16 or f32 [N,C] (unit
    channel stride, any row stride >= C), 1 <= C <= 4096.  ``out``: a f16 or f32 [H,W,C] tensor on the rows' GPU with a unit
    channel stride and any pixel stride >= C (elements C.. of a pixel are not touched), or None for a fresh contiguous one
    of ``dtype``.  The default ``dtype=None`` stands for torch.float16 (the fp32 sums rounded once; above 65504 they become
    Inf): this module imports torch inside its functions, so the default cannot name torch.float16, and None also lets
    ``out=`` alone decide the format.  ``sorted``: False sorts
    ``capacity`` keys first (valid directly after splat_project; the workspace grows as for splat_rasterize), True reuses
    the sort a splat_rasterize / splat_rasterize_loss / splat_lift / splat_render call with the same capacity left.
    ``status``: optional device int32 [1], set to 1 when the device count exceeds ``capacity`` (then nothing is written).
    With ``check`` the call reads the status word (one synchronisation) and raises VoxprojError when it is set.
    Returns (out, alpha f32 [H,W] or None); alpha is bit-identical to splat_rasterize's."""
    import torch
    _require(isinstance(sorted, (bool, int)) and int(sorted) in (0, 1), "sorted must be False or True")
    _require_tensors((rows, "rows", (torch.float16, torch.float32)))
    dev, N = rows.device, int(n_gaussians)
    _require(rows.dim() == 2 and int(rows.shape[0]) == N, f"rows must be [{N}, C]")
    C = int(rows.shape[1])
    _require(1 <= C <= 4096, f"C = {C} outside [1, 4096]")
    if N and (rows.stride(1) != 1 or (N > 1 and rows.stride(0) < C)):
        rows = rows.contiguous()
    if out is None:
        out = torch.empty((int(H), int(W), C), dtype=torch.float16 if dtype is None else dtype, device=dev)
    else:
        _require(dtype is None or out.dtype == dtype, "out and dtype disagree")
    _require_tensors((out, "out", (torch.float16, torch.float32)))
    _require(out.device == dev and tuple(out.shape) == (int(H), int(W), C) and out.stride(2) == 1 and out.stride(1) >= C and
             out.stride(0) == int(W) * out.stride(1),
             f"out must be [{H}, {W}, {C}] on the rows' device, channels-last with one pixel stride >= C")
    if status is None and check:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    if status is not None:
        _require_tensors((status, "status", (torch.int32,)))
        _require(status.numel() == 1 and status.device == dev, "status must be one int32 on the rows' device")
    if sorted:
        ptr = _filled_workspace("splat_render(sorted=True)", "splat_rasterize", workspace,
                                _splat_workspace_bytes(N, W, H, capacity), dev)
    else:
        ptr = _splat_forward_workspace(workspace, N, W, H, capacity, dev)
    alpha = torch.empty((int(H), int(W)), dtype=torch.float32, device=dev) if want_alpha else None
    _call(dev, "vp_splat_render", rows.data_ptr() if N else ptr, int(rows.dtype == torch.float16), C,
          max(int(rows.stride(0)), C) if N > 1 else C, N, int(W), int(H), int(capacity), int(sorted), out.data_ptr(),
          int(out.dtype == torch.float16), int(out.stride(1)), _ptr(alpha), _ptr(status), ptr, workspace.capacity())
    if check and int(status.item()):
        raise VoxprojError("splat_render: the intersection count outgrew the workspace (nothing written)")
    return out, alpha


def splat_render_view(means, quats, scales, opacities, rows, viewmat, K, W, H, *, out=None, dtype=None, want_alpha=False,
                      near=0.01, far=1e10, eps2d=0.3, workspace=None, check=True):
    """Render the Gaussians' wide rows into one view (vp_splat_project + vp_splat_render), as splat_features splats logits:
    reads the 8-byte intersection count once to size the sort.  Returns (out [H,W,C], alpha f32 [H,W] or None, n_isect int,
    n_nonfinite device int32 [1]); ``out`` / ``dtype`` as in splat_render.  With ``check`` the call synchronises once more
    and raises VoxprojError when a Gaussian had a non-finite parameter (it is culled)."""
    import torch
    _require_tensors(*((t, name, (torch.float32,)) for t, name in
                       ((means, "means"), (quats, "quats"), (scales, "scales"), (opacities, "opacities"))))
    _require(isinstance(rows, torch.Tensor) and rows.device == means.device, "rows and the Gaussians must be on one device")
    ws, cap, bad, status = _splat_sized_view(means, quats, scales, opacities, viewmat, K, W, H, near, far, eps2d, workspace)
    out, alpha = splat_render(rows, int(means.shape[0]), W, H, cap, ws, out=out, dtype=dtype, want_alpha=want_alpha,
                              sorted=False, status=status, check=False)
    if check:
        _splat_view_check("splat_render_view", status, bad, "nothing written")
    return out, alpha, cap, bad


FEATURE_LOSS_KINDS = {"cosine": VP_FEATURE_LOSS_COSINE, "l2": VP_FEATURE_LOSS_L2}


def feature_loss_workspace_bytes(W, H):
    """vp_feature_loss_workspace_bytes: bytes of the feature loss's workspace for a W x H view (0 when out of range).  Needs
    no GPU."""
    return int(_entry("vp_feature_loss_workspace_bytes")(int(W), int(H)))


def _feature_maps(caller, image, target):
    """The image f16 / f32 [H,W,C] and the map f16 [H,W,C] of the feature loss on one GPU, channels-last with a unit channel
    stride and one pixel stride >= C each (a contiguous copy otherwise): (image, target, H, W, C)."""
    import torch
    _require_tensors((image, "image", (torch.float16, torch.float32)), (target, "target", (torch.float16,)))
    _require(image.dim() == 3 and image.numel() > 0, "image must be [H, W, C]")
    H, W, C = (int(v) for v in image.shape)
    _require(1 <= C <= 4096, f"C = {C} outside [1, 4096]")
    _require(1 <= W <= 32768 and 1 <= H <= 32768, f"image size {W} x {H} outside [1, 32768]")
    _require(tuple(target.shape) == (H, W, C) and target.device == image.device,
             f"{caller}: target must be float16 [{H}, {W}, {C}] on the image's device")

    def layout(t):
        return t if t.stride(2) == 1 and t.stride(1) >= C and t.stride(0) == W * t.stride(1) else t.contiguous()
    return layout(image), layout(target), H, W, C


def feature_loss(image, target, pixel_weight=None, alpha=None, *, kind="cosine", min_alpha=0.0, want_pixel_loss=False,
                 workspace=None):
    """vp_feature_loss: the cosine or L2 loss of a rendered feature image against a 2D feature map, per pixel and summed.
    image f16 or f32 [H,W,C] (what splat_render writes), target f16 [H,W,C] (what upsample_features(keep_dtype=True) returns
    for an f16 map), both channels-last with a unit channel stride and any pixel stride >= C, on one GPU.  pixel_weight f32
    [H,W] or None (1; a value that is not > 0 reads as 0), alpha f32 [H,W] or None with ``min_alpha``: a pixel is valid when
    its weight is > 0, alpha >= min_alpha and, for "cosine", neither row is all zeros.  ``workspace``: a SplatWorkspace that
    the call fills for feature_loss_gradient (a fresh one when None).
    Returns (loss_stats f64 [2] = {sum m l, sum m}, pixel_loss f32 [H,W] or None, workspace); nothing is read back here."""
    import torch
    _require(kind in FEATURE_LOSS_KINDS, f"kind must be 'cosine' or 'l2', not {kind!r}")
    image, target, H, W, C = _feature_maps("feature_loss", image, target)
    dev = image.device
    pixel_weight, alpha = _splat_images(dev, (pixel_weight, "pixel_weight", (H, W), torch.float32),
                                        (alpha, "alpha", (H, W), torch.float32))
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(feature_loss_workspace_bytes(W, H), dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    pixel_loss = torch.empty((H, W), dtype=torch.float32, device=dev) if want_pixel_loss else None
    _call(dev, "vp_feature_loss", image.data_ptr(), int(image.dtype == torch.float16), int(image.stride(1)), target.data_ptr(),
          int(target.stride(1)), C, W, H, _ptr(pixel_weight), _ptr(alpha), float(min_alpha), FEATURE_LOSS_KINDS[kind],
          stats.data_ptr(), _ptr(pixel_loss), ptr, ws.capacity())
    return stats, pixel_loss, ws


def feature_loss_gradient(image, target, loss_stats, workspace, *, reduction="mean", grad_loss=None, out=None):
    """vp_feature_loss_gradient after feature_loss on ``workspace`` with the same image and target: the gradient image of the
    loss in binary16 with one exponent for the map, the form splat_lift reads.  ``reduction`` "mean" (the scalar is
    grad_loss / sum m, formed on the device from ``loss_stats``; sum m = 0 gives zeros) or "sum"; ``grad_loss``: a device f32
    [1] (None: 1).  ``out``: a f16 [H,W,C] tensor with a unit channel stride and one pixel stride >= C (elements C.. of a
    pixel are not touched), or None for a fresh contiguous one.
    Returns (Gq f16 [H,W,C], k int32 [1] on the device): the gradient is Gq / 2^k; nothing is read back here."""
    import torch
    _require(reduction in _REDUCTIONS, f"reduction must be 'mean' or 'sum', not {reduction!r}")
    image, target, H, W, C = _feature_maps("feature_loss_gradient", image, target)
    dev = image.device
    _require_tensors((loss_stats, "loss_stats", (torch.float64,)))
    _require(loss_stats.numel() == 2 and loss_stats.device == dev and loss_stats.is_contiguous(),
             "loss_stats must be the float64 [2] tensor feature_loss returned")
    (grad_loss,) = _splat_images(dev, (grad_loss, "grad_loss", None, torch.float32))
    ptr = _filled_workspace("feature_loss_gradient", "feature_loss", workspace, feature_loss_workspace_bytes(W, H), dev)
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.float16, device=dev)
    _require_tensors((out, "out", (torch.float16,)))
    _require(out.device == dev and tuple(out.shape) == (H, W, C) and out.stride(2) == 1 and out.stride(1) >= C and
             out.stride(0) == W * out.stride(1), f"out must be float16 [{H}, {W}, {C}], channels-last with one pixel stride >= C")
    k = torch.empty(1, dtype=torch.int32, device=dev)
    _call(dev, "vp_feature_loss_gradient", image.data_ptr(), int(image.dtype == torch.float16), int(image.stride(1)),
          target.data_ptr(), int(target.stride(1)), C, W, H, loss_stats.data_ptr(), _REDUCTIONS[reduction], _ptr(grad_loss),
          out.data_ptr(), int(out.stride(1)), k.data_ptr(), ptr, workspace.capacity())
    return out, k


VP_PROTO_MAX_IDS = 256


def proto_contrast_workspace_bytes(D, W, H):
    """vp_proto_contrast_workspace_bytes: bytes of the prototype-contrastive loss's workspace for a D-channel W x H image
    (0 when out of range).  Needs no GPU."""
    return int(_entry("vp_proto_contrast_workspace_bytes")(int(D), int(W), int(H)))


def _gradient_image(out, shape, dev):
    """The contiguous f32 image of ``shape`` on ``dev`` a gradient call writes: a fresh one, or the caller's ``out`` checked."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    _require_tensors((out, "out", (torch.float32,)))
    _require(out.device == dev and tuple(out.shape) == shape and out.is_contiguous(),
             f"out must be a contiguous float32 [{shape[0]}, {shape[1]}, {shape[2]}] tensor on the image's device")
    return out


def _proto_maps(caller, image, ids, count):
    """The image f32 [D,H,W], the mask i32 [H,W] and the multiplicity map i32 [H,W] or None, contiguous on one GPU."""
    import torch
    _require_tensors((image, "image", (torch.float32,)), (ids, "ids", (torch.int32,)))
    _require(image.dim() == 3 and image.numel() > 0, "image must be [D, H, W]")
    D, H, W = (int(v) for v in image.shape)
    _require(1 <= D <= 64, f"D = {D} outside [1, 64]")
    _require(1 <= W <= 32768 and 1 <= H <= 32768, f"image size {W} x {H} outside [1, 32768]")
    dev = image.device
    _require(tuple(ids.shape) == (H, W) and ids.device == dev, f"{caller}: ids must be int32 [{H}, {W}] on the image's device")
    (count,) = _splat_images(dev, (count, "count", (H, W), torch.int32))
    return image.contiguous(), ids.contiguous(), count, D, H, W


def proto_contrast(image, ids, count=None, *, ignore_id=-1, min_count=20, phi_scale=10.0, phi_min=0.5, phi_max=1.0,
                   want_pixel_loss=False, want_own_prob=False, workspace=None):
    """vp_proto_contrast: the prototype-contrastive loss of a rendered identity image against one view's instance mask.
    image f32 [D,H,W] (splat_features' logits), ids int32 [H,W], count int32 [H,W] or None (every pixel drawn once), on one
    GPU.  The defaults are the loss's parameters; phi_scale 0.1, phi_min 0.1, min_count 0 are the confidence map's.
    ``workspace``: a SplatWorkspace the call fills for proto_contrast_gradient (a fresh one when None).
    Returns (stats f64 [4] = {sum m l, K, sum (r - 1)^2, sum m}, pixel_loss f32 [H,W] or None, own_prob f32 [H,W] or None,
    workspace); nothing is read back here."""
    import torch
    image, ids, count, D, H, W = _proto_maps("proto_contrast", image, ids, count)
    dev = image.device
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(proto_contrast_workspace_bytes(D, W, H), dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    pixel_loss = torch.empty((H, W), dtype=torch.float32, device=dev) if want_pixel_loss else None
    own_prob = torch.empty((H, W), dtype=torch.float32, device=dev) if want_own_prob else None
    _call(dev, "vp_proto_contrast", image.data_ptr(), D, W, H, ids.data_ptr(), _ptr(count), int(ignore_id), int(min_count),
          float(phi_scale), float(phi_min), float(phi_max), stats.data_ptr(), _ptr(pixel_loss), _ptr(own_prob), ptr,
          ws.capacity())
    return stats, pixel_loss, own_prob, ws


def proto_contrast_gradient(image, ids, count, workspace, *, weight_contrast=1.0, weight_norm=1.0, grad_loss=None, out=None):
    """vp_proto_contrast_gradient after proto_contrast on ``workspace`` with the same image, ids and count: the gradient
    image f32 [D,H,W] of  weight_contrast (sum m l) / K + weight_norm (sum (r - 1)^2) / (W H), times ``grad_loss`` (a device
    f32 [1]; None: 1).  ``out``: a contiguous f32 [D,H,W] tensor, or None for a fresh one.  Nothing is read back here."""
    import torch
    image, ids, count, D, H, W = _proto_maps("proto_contrast_gradient", image, ids, count)
    dev = image.device
    (grad_loss,) = _splat_images(dev, (grad_loss, "grad_loss", None, torch.float32))
    ptr = _filled_workspace("proto_contrast_gradient", "proto_contrast", workspace, proto_contrast_workspace_bytes(D, W, H), dev)
    out = _gradient_image(out, (D, H, W), dev)
    _call(dev, "vp_proto_contrast_gradient", image.data_ptr(), D, W, H, ids.data_ptr(), _ptr(count), float(weight_contrast),
          float(weight_norm), _ptr(grad_loss), out.data_ptr(), ptr, workspace.capacity())
    return out


def photo_loss_workspace_bytes(C, W, H):
    """vp_photo_loss_workspace_bytes: bytes of the photometric loss's workspace for a C-channel W x H image (0 when out of
    range).  Needs no GPU."""
    return int(_entry("vp_photo_loss_workspace_bytes")(int(C), int(W), int(H)))


def _photo_maps(caller, image, target):
    """The rendered image and the photograph, f32 [C,H,W], contiguous on one GPU."""
    import torch
    _require_tensors((image, "image", (torch.float32,)), (target, "target", (torch.float32,)))
    _require(image.dim() == 3 and image.numel() > 0, "image must be [C, H, W]")
    C, H, W = (int(v) for v in image.shape)
    _require(1 <= C <= 64, f"C = {C} outside [1, 64]")
    _require(1 <= W <= 32768 and 1 <= H <= 32768, f"image size {W} x {H} outside [1, 32768]")
    _require(tuple(target.shape) == (C, H, W) and target.device == image.device,
             f"{caller}: target must be float32 [{C}, {H}, {W}] on the image's device")
    return image.contiguous(), target.contiguous(), C, H, W


def photo_loss(image, target, *, want_ssim_map=False, workspace=None, evaluate_only=False):
    """vp_photo_loss: the L1 / squared-error / SSIM sums of a rendered image against a photograph, both f32 [C,H,W] on one
    GPU (image: splat_features' logits).  ``workspace``: a SplatWorkspace the call fills for photo_loss_gradient (a fresh one
    when None).  ``evaluate_only``: no workspace at all -- the same stats bits, nothing kept for a gradient, and the image is
    walked by one workgroup.
    Returns (stats f64 [3] = {sum |x - y|, sum (x - y)^2, sum m}, ssim_map f32 [C,H,W] or None, workspace or None); nothing
    is read back here."""
    import torch
    image, target, C, H, W = _photo_maps("photo_loss", image, target)
    dev = image.device
    _require(not (evaluate_only and workspace is not None), "photo_loss: evaluate_only takes no workspace")
    ws, ptr, cap = None, None, 0
    if not evaluate_only:
        ws = workspace if workspace is not None else SplatWorkspace()
        ptr = ws.ensure(photo_loss_workspace_bytes(C, W, H), dev)
        cap = ws.capacity()
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    ssim_map = torch.empty((C, H, W), dtype=torch.float32, device=dev) if want_ssim_map else None
    _call(dev, "vp_photo_loss", image.data_ptr(), target.data_ptr(), C, W, H, stats.data_ptr(), _ptr(ssim_map), ptr, cap)
    return stats, ssim_map, ws


def photo_loss_gradient(image, target, workspace, *, lambda_dssim, grad_loss=None, out=None):
    """vp_photo_loss_gradient after photo_loss on ``workspace`` with the same image and target: the gradient image f32
    [C,H,W] of  (1 - lambda_dssim) mean |x - y| + lambda_dssim (1 - mean m), times ``grad_loss`` (a device f32 [1]; None: 1).
    ``out``: a contiguous f32 [C,H,W] tensor, or None for a fresh one.  Nothing is read back here."""
    import torch
    image, target, C, H, W = _photo_maps("photo_loss_gradient", image, target)
    dev = image.device
    (grad_loss,) = _splat_images(dev, (grad_loss, "grad_loss", None, torch.float32))
    ptr = _filled_workspace("photo_loss_gradient", "photo_loss", workspace, photo_loss_workspace_bytes(C, W, H), dev)
    out = _gradient_image(out, (C, H, W), dev)
    _call(dev, "vp_photo_loss_gradient", image.data_ptr(), target.data_ptr(), C, W, H, float(lambda_dssim), _ptr(grad_loss),
          out.data_ptr(), ptr, workspace.capacity())
    return out


def image_metrics(stats, n):
    """{l1, psnr, ssim} as Python floats from photo_loss's stats (a tensor or three numbers; a tensor is read back here) and
    n = C W H.  psnr is inf for identical images."""
    import math
    s = [float(v) for v in (stats.tolist() if hasattr(stats, "tolist") else stats)]
    mse = s[1] / n
    return {"l1": s[0] / n, "psnr": -10.0 * math.log10(mse) if mse > 0.0 else math.inf, "ssim": s[2] / n}


class _DensifyArray(ctypes.Structure):
    """vp_densify_array of include/voxproj.h."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("width", ctypes.c_int32), ("fill", ctypes.c_int32),
                ("src_stride", ctypes.c_int64), ("dst_stride", ctypes.c_int64)]


_DENSIFY_FILLS = {"copy": VP_DENSIFY_COPY, "zero": VP_DENSIFY_ZERO}


def _densify_lib():
    """The library, for the GPU tests that drive the densification entry points through the C ABI themselves."""
    _entry("vp_densify_plan")
    return lib()


def camera_extent(viewmats):
    """1.1 max |c_i - mean c| over the camera centres c = -R^T t of world-to-camera matrices [V,4,4] (any device, read on the
    host, float64): the reference's cameras_extent, the length the densification's size thresholds are stated in."""
    import numpy as np
    import torch
    vm = np.stack([torch.as_tensor(v, dtype=torch.float64).detach().cpu().numpy().reshape(4, 4) for v in viewmats])
    c = -np.einsum("nji,nj->ni", vm[:, :3, :3], vm[:, :3, 3])
    return float(1.1 * np.linalg.norm(c - c.mean(0), axis=1).max())


class DensifyStats:
    """The running statistics of adaptive density control for n Gaussians on ``device``: grad_accum f32 [n], denom i32 [n]
    and, with ``want_radius``, max_radius f32 [n] (None otherwise).  ``reset(n)`` starts over at a new size."""

    def __init__(self, n, device, want_radius=False):
        self.device = device
        self.want_radius = bool(want_radius)
        self.reset(n)

    def reset(self, n):
        import torch
        self.n = int(n)
        self.grad_accum = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.denom = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.max_radius = torch.zeros(self.n, dtype=torch.float32, device=self.device) if self.want_radius else None


def densify_accumulate(stats, grad_screen, workspace, W, H, scale=1.0, geometry=None):
    """vp_densify_accumulate: add one view to ``stats``.  grad_screen f32 [N,5] from the geometry backward of the view
    (want_screen=True), ``workspace`` the SplatWorkspace of its splat_project / splat_rasterize (only read); ``scale`` undoes a
    caller's 1 / k.  ``geometry``: (means, quats, scales, viewmat, K) or (..., eps2d) of the project call, needed when the
    stats keep max_radius and ignored otherwise.  Asynchronous; nothing is read back."""
    import torch
    _require_tensors((grad_screen, "grad_screen", (torch.float32,)))
    N = stats.n
    dev = grad_screen.device
    _require(tuple(grad_screen.shape) == (N, 5) and grad_screen.is_contiguous(), f"grad_screen must be a contiguous [{N}, 5]")
    _require(stats.grad_accum.device == dev, "the statistics and grad_screen must be on one device")
    _require(1 <= int(W) <= 32768 and 1 <= int(H) <= 32768, f"image size {W} x {H} outside [1, 32768]")
    ptr = _filled_workspace("densify_accumulate", "splat_project", workspace,
                            int(lib().vp_splat_workspace_bytes(N, int(W), int(H), 0)), dev)
    m = q = s = vm = None
    fx = fy = cx = cy = 0.0
    eps2d = 0.3
    if stats.max_radius is not None:
        _require(geometry is not None and len(geometry) in (5, 6),
                 "densify_accumulate: statistics with max_radius need geometry = (means, quats, scales, viewmat, K[, eps2d])")
        _, (m, q, s) = _splat_gaussians(geometry[0].detach(), geometry[1].detach(), geometry[2].detach(), dev=dev)
        _require(int(m.shape[0]) == N, f"the geometry must have {N} Gaussians")
        vm, (fx, fy, cx, cy) = _splat_camera(geometry[3], geometry[4], W, H)
        if len(geometry) == 6:
            eps2d = float(geometry[5])
    _call(dev, "vp_densify_accumulate", _ptr(grad_screen), N, int(W), int(H), float(scale), _ptr(m), _ptr(q), _ptr(s), vm, fx,
          fy, cx, cy, eps2d, _ptr(stats.grad_accum), _ptr(stats.denom), _ptr(stats.max_radius), ptr, workspace.capacity())


def densify_rows(arrays, src, kind, counts, n_src, n_out, status=None):
    """vp_densify_rows, at most 16 arrays per launch (more are sent in several): ``arrays`` is a list of (src tensor, dst
    tensor, fill) with 32-bit tensors whose rows are the first dimension: contiguous, or 2-D with a unit element stride and a
    row stride >= the width.  dst row r = src row src[r] (zeros where fill is "zero" and kind[r] != 0).  ``n_out`` is the
    host's copy of counts[0]; when the device disagrees nothing is written and ``status`` (device int32 [1]) becomes 1."""
    import torch
    descs = []
    for a, d, fill in arrays:
        _require_tensors((a, "a source array", (torch.float32, torch.int32)), (d, "a destination array", (a.dtype,)))
        _require(fill in _DENSIFY_FILLS, f"fill must be 'copy' or 'zero', not {fill!r}")
        _require(a.dim() >= 1 and d.dim() == a.dim() and int(a.shape[0]) == int(n_src) and int(d.shape[0]) == int(n_out) and
                 tuple(a.shape[1:]) == tuple(d.shape[1:]) and a.device == src.device and d.device == src.device,
                 "an array must be [n_src, ...] and its destination [n_out, ...] with the same row shape, on the plan's device")
        width = 1
        for v in a.shape[1:]:
            width *= int(v)
        strides = []
        for t in (a, d):
            if t.is_contiguous():
                strides.append(width)
            else:
                _require(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1],
                         "a strided array must be 2-D with a unit element stride and a row stride >= its width")
                strides.append(int(t.stride(0)))
        _require(1 <= width <= VP_DENSIFY_MAX_WIDTH, f"a row has {width} words: outside [1, {VP_DENSIFY_MAX_WIDTH}]")
        descs.append(_DensifyArray(_ptr(a), _ptr(d), width, _DENSIFY_FILLS[fill], strides[0], strides[1]))
    for i in range(0, len(descs), VP_DENSIFY_MAX_ARRAYS):
        part = descs[i:i + VP_DENSIFY_MAX_ARRAYS]
        _call(src.device, "vp_densify_rows", (_DensifyArray * len(part))(*part), len(part), _ptr(src), _ptr(kind),
              counts.data_ptr(), int(n_src), int(n_out), _ptr(status))


class DensifyPlan:
    """What vp_densify_plan decided: src i32 [2N] and kind u8 [2N] (rows [0, n_out) are meaningful) and counts i64 [4] on the
    device; n_out, kept, clones, split (splitting sources) as Python ints; status, a device int32 [1] that a resample or split
    call raises when its n_out is not the device's."""

    def __init__(self, n, src, kind, counts, status):
        self.n, self.src, self.kind, self.counts, self.status = int(n), src, kind, counts, status
        self.n_out, self.kept, self.clones, self.split = (int(v) for v in counts.tolist())

    def resample(self, arrays):
        """{name: (tensor [N, ...] f32 or i32, "copy" | "zero")} -> {name: the new tensor [n_out, ...]}, one launch per 16
        arrays.  "zero" fills the rows that are not kept originals with zeros (optimiser moments)."""
        import torch
        out, todo = {}, []
        for name, (t, fill) in arrays.items():
            _require(isinstance(t, torch.Tensor) and t.dim() >= 1 and int(t.shape[0]) == self.n,
                     f"{name} must be a tensor with {self.n} rows")
            t = t.detach()
            if not t.is_contiguous():
                t = t.contiguous()
            out[name] = torch.empty((self.n_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            if self.n_out and out[name].numel():
                todo.append((t, out[name], fill))
        if todo:
            densify_rows(todo, self.src, self.kind, self.counts, self.n, self.n_out, self.status)
        return out

    def split_geometry(self, means, quats, log_scales, seed):
        """vp_densify_split: (means f32 [n_out,3], log_scales f32 [n_out,3]) of the new cloud: copies for kept rows and
        clones, sampled positions and shrunk scales for the split children.  ``seed``: an int below 2^64 or (low, high)
        32-bit words; the same seed and inputs give the same bits."""
        import torch
        _, (m, q, s) = _splat_gaussians(means.detach(), quats.detach(), log_scales.detach())
        _require(int(m.shape[0]) == self.n and m.device == self.src.device, f"the geometry must have {self.n} Gaussians")
        if isinstance(seed, (tuple, list)):
            seed = (int(seed[0]) & 0xFFFFFFFF) | ((int(seed[1]) & 0xFFFFFFFF) << 32)
        _require(0 <= int(seed) < 2 ** 64, "seed must be in [0, 2^64)")
        dev = m.device
        om = torch.empty((self.n_out, 3), dtype=torch.float32, device=dev)
        ol = torch.empty((self.n_out, 3), dtype=torch.float32, device=dev)
        _call(dev, "vp_densify_split", _ptr(m), _ptr(q), _ptr(s), self.n, _ptr(self.src), _ptr(self.kind),
              self.counts.data_ptr(), self.n_out, int(seed), _ptr(om), _ptr(ol), _ptr(self.status))
        return om, ol


def densify_plan(stats, scales, opacities, *, grad_threshold, size_threshold, min_opacity, max_screen_size=0.0, max_world_size,
                 workspace=None):
    """vp_densify_plan: the clone / split / prune decision of every Gaussian from ``stats`` and the activated scales f32 [N,3]
    and opacities f32 [N], and the source row of every output row.  size_threshold = percent_dense x extent, max_world_size =
    0.1 x extent; max_screen_size 0 turns the size rules off.  Reads the four counters back: the one synchronisation of a
    densification.  ``workspace``: a SplatWorkspace for the scan's scratch (a fresh one when None)."""
    import torch
    _require_tensors((scales, "scales", (torch.float32,)), (opacities, "opacities", (torch.float32,)))
    N, dev = stats.n, scales.device
    _require(tuple(scales.shape) == (N, 3) and tuple(opacities.shape) == (N,), f"scales must be [{N}, 3] and opacities [{N}]")
    _require(opacities.device == dev and stats.grad_accum.device == dev, "the statistics, scales and opacities must be on one device")
    _require(float(grad_threshold) > 0.0, f"grad_threshold = {grad_threshold} must be > 0")
    scales, opacities = scales.detach().contiguous(), opacities.detach().contiguous()
    need = int(_entry("vp_densify_plan_workspace_bytes")(N))
    _require(need > 0, f"no plan workspace size for N = {N}")
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(need, dev)
    src = torch.empty(2 * N, dtype=torch.int32, device=dev)
    kind = torch.empty(2 * N, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _call(dev, "vp_densify_plan", _ptr(stats.grad_accum), _ptr(stats.denom), _ptr(stats.max_radius), _ptr(scales),
          _ptr(opacities), N, float(grad_threshold), float(size_threshold), float(min_opacity), float(max_screen_size),
          float(max_world_size), _ptr(src), _ptr(kind), counts.data_ptr(), ptr, ws.capacity())
    return DensifyPlan(N, src, kind, counts, status)


def resample_adam(optimizer, old_params, new_params, plan):
    """Replace the parameters {name: old_param} of a torch.optim.Adam by {name: new_param} (resampled by ``plan``) in their
    groups, and carry exp_avg / exp_avg_sq over in one resample call: the surviving rows keep their moments bit for bit, new
    rows start at zero, ``step`` is kept (the reference's _prune_optimizer and cat_tensors_to_optimizer together)."""
    moments, states = {}, {}
    for name, old in old_params.items():
        new = new_params[name]
        for group in optimizer.param_groups:
            for i, q in enumerate(group["params"]):
                if q is old:
                    group["params"][i] = new
        st = optimizer.state.pop(old, None)
        if st:
            states[name] = st
            for key in ("exp_avg", "exp_avg_sq"):
                if key in st:
                    moments[(name, key)] = (st[key], "zero")
    moved = plan.resample(moments) if moments else {}
    for name, st in states.items():
        for key in ("exp_avg", "exp_avg_sq"):
            if (name, key) in moved:
                st[key] = moved[(name, key)]
        optimizer.state[new_params[name]] = st


def _mesh_arrays(verts, faces, vertex_labels=None):
    """The float32 [V,3] vertices, int32 [F,3] faces and optional uint8 [V] labels on one GPU, contiguous: (V, F, arrays)."""
    import torch
    specs = [(verts, "verts", (torch.float32,)), (faces, "faces", (torch.int32,))]
    if vertex_labels is not None:
        specs.append((vertex_labels, "vertex_labels", (torch.uint8,)))
    _require_tensors(*specs)
    _require(verts.dim() == 2 and int(verts.shape[1]) == 3, "verts must be [V, 3]")
    _require(faces.dim() == 2 and int(faces.shape[1]) == 3, "faces must be [F, 3]")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    _require(vertex_labels is None or tuple(vertex_labels.shape) == (V,), f"vertex_labels must be [{V}]")
    _require(all(t.device == verts.device for t, _, _ in specs), "the mesh tensors must be on one device")
    return V, F, [t.contiguous() for t, _, _ in specs]


def _mesh_workspace_bytes(n_faces, W, H, capacity):
    nbytes = int(_entry("vp_mesh_workspace_bytes")(int(n_faces), int(W), int(H), int(capacity)))
    _require(nbytes > 0, f"no workspace size for {n_faces} faces, {W} x {H}, capacity {capacity}")
    return nbytes


def mesh_project(verts, faces, viewmat, K, W, H, *, near=0.01, far=100.0, workspace=None, counters=None):
    """vp_mesh_project (the contract is in include/voxproj_mesh.h): every face of the mesh set up once into ``workspace`` (a
    SplatWorkspace; grown to the projection's size).  verts f32 [V,3] and faces i32 [F,3] on one GPU, viewmat [4,4]
    world-to-camera and K [3,3] (read on the host), as for splat_project.  Returns the device int64 [1] count of (tile, face)
    pairs (not read here).  ``counters``: optional device int32 [3], += the faces dropped for {an index outside the vertices,
    a non-finite vertex, a coordinate beyond the guard band}."""
    import torch
    V, F, (verts, faces) = _mesh_arrays(verts, faces)
    dev = verts.device
    vm, (fx, fy, cx, cy) = _splat_camera(viewmat, K, W, H)
    _require(0.0 < float(near) < float(far) < float("inf"), f"need 0 < near < far (got {near}, {far})")
    if counters is not None:
        _require_tensors((counters, "counters", (torch.int32,)))
        _require(tuple(counters.shape) == (3,) and counters.device == dev and counters.is_contiguous(),
                 "counters must be a contiguous int32 [3] on the mesh's device")
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(_mesh_workspace_bytes(F, W, H, 0), dev)
    n_isect = torch.zeros(1, dtype=torch.int64, device=dev)
    _call(dev, "vp_mesh_project", _ptr(verts), V, _ptr(faces), F, vm, fx, fy, cx, cy, int(W), int(H), float(near), float(far),
          n_isect.data_ptr(), _ptr(counters), ptr, ws.capacity())
    return n_isect


def mesh_rasterize(faces, vertex_labels, W, H, capacity, workspace, *, want_depth=True, want_labels=True, status=None, out=None):
    """vp_mesh_rasterize after mesh_project on ``workspace`` with the same faces, W and H: sort ``capacity`` (tile, face)
    pairs and run the tile kernel.  The workspace grows to ``capacity`` (the projection's bytes kept).  Returns (face_ids int32
    [H,W], depth f32 [H,W] or None, labels uint8 [H,W] or None); ``out``: three tensors (or None) to write instead of new
    ones.  ``vertex_labels`` uint8 [V] may be None without labels.  ``status``: optional device int32 [1], set to 1 when the
    device count exceeds ``capacity`` (then no output is written)."""
    import torch
    _require_tensors((faces, "faces", (torch.int32,)))
    _require(faces.dim() == 2 and int(faces.shape[1]) == 3, "faces must be [F, 3]")
    faces = faces.contiguous()
    F, dev = int(faces.shape[0]), faces.device
    want_labels = bool(want_labels and vertex_labels is not None)
    if want_labels:
        _require_tensors((vertex_labels, "vertex_labels", (torch.uint8,)))
        _require(vertex_labels.dim() == 1 and vertex_labels.device == dev, "vertex_labels must be uint8 [V] on the faces' device")
        vertex_labels = vertex_labels.contiguous()
    _filled_workspace("mesh_rasterize", "mesh_project", workspace, _mesh_workspace_bytes(F, W, H, 0), dev)
    ptr = _splat_forward_workspace(workspace, F, W, H, capacity, dev, _mesh_workspace_bytes)
    if out is None:
        out = (torch.empty((H, W), dtype=torch.int32, device=dev),
               torch.empty((H, W), dtype=torch.float32, device=dev) if want_depth else None,
               torch.empty((H, W), dtype=torch.uint8, device=dev) if want_labels else None)
    ids, depth, labels = _splat_images(dev, (out[0], "face_ids", (H, W), torch.int32), (out[1], "depth", (H, W), torch.float32),
                                       (out[2], "labels", (H, W), torch.uint8))
    _require(labels is None or want_labels, "labels need vertex_labels")
    _call(dev, "vp_mesh_rasterize", _ptr(vertex_labels) if want_labels else None, _ptr(faces), F, int(W), int(H), int(capacity),
          _ptr(ids), _ptr(depth), _ptr(labels), _ptr(status), ptr, workspace.capacity())
    return ids, depth, labels


def mesh_render(verts, faces, vertex_labels, viewmat, K, W, H, near=0.01, far=100.0, workspace=None):
    """Rasterize an annotated triangle mesh into one W x H view (vp_mesh_project + vp_mesh_rasterize): per pixel the nearest
    face, its depth and the majority label of its vertices, at the splatter's camera and pixel centres.  Reads the 8-byte pair
    count once to size the sort, as splat_features does (``workspace``: a SplatWorkspace, kept and regrown across calls).
    Returns (face_ids int32 [H,W], -1 where nothing is drawn; depth f32 [H,W], 0 there; labels uint8 [H,W], 255 there, None
    without vertex_labels; counters int32 [3] on the device: the faces dropped for a bad index, a non-finite vertex, the
    guard band)."""
    import torch
    _mesh_arrays(verts, faces, vertex_labels)
    dev = verts.device
    ws = workspace if workspace is not None else SplatWorkspace()
    counters = torch.zeros(3, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_isect = mesh_project(verts, faces, viewmat, K, W, H, near=near, far=far, workspace=ws, counters=counters)
    cap = int(n_isect.item())
    _require(cap <= 2 ** 31 - 1, f"{cap} tile intersections: more than 2^31 - 1")
    ids, depth, labels = mesh_rasterize(faces, vertex_labels, W, H, cap, ws, status=status)
    if int(status.item()):
        raise VoxprojError("mesh_render: the pair count outgrew the workspace (no image written)")
    return ids, depth, labels, counters


def camera_position(viewmat):
    """The camera centre -R^T t of a [4,4] world-to-camera matrix (any device, read on the host), in float64: three floats."""
    import torch
    vm = torch.as_tensor(viewmat, dtype=torch.float64).detach().cpu().reshape(-1)
    _require(vm.numel() == 16, "viewmat must be a [4, 4] world-to-camera matrix")
    vm = vm.reshape(4, 4)
    return [float(v) for v in -(vm[:3, :3].T @ vm[:3, 3])]


def sh_rest_width(max_degree):
    """Kr = (max_degree + 1)^2 - 1, the coefficient rows of f_rest."""
    _require(0 <= int(max_degree) <= VP_SH_MAX_DEGREE, f"SH degree {max_degree} outside [0, {VP_SH_MAX_DEGREE}]")
    return (int(max_degree) + 1) ** 2 - 1


def _sh_inputs(caller, f_dc, f_rest, means, degree):
    """f_dc [N,3], f_rest [N,Kr,3] with Kr = (Dmax + 1)^2 - 1 for a Dmax <= 3, means [N,3], float32 on one GPU, and an active
    degree <= Dmax: (N, Dmax, contiguous tensors).  Views that are contiguous but start inside a buffer stay views."""
    import torch
    _require_tensors((f_dc, "f_dc", (torch.float32,)), (f_rest, "f_rest", (torch.float32,)), (means, "means", (torch.float32,)))
    N = int(f_dc.shape[0]) if f_dc.dim() == 2 else -1
    _require(N >= 0 and tuple(f_dc.shape) == (N, 3), f"{caller}: f_dc must be [N, 3]")
    _require(tuple(means.shape) == (N, 3), f"{caller}: means must be [{N}, 3]")
    _require(f_rest.dim() == 3 and int(f_rest.shape[0]) == N and int(f_rest.shape[2]) == 3, f"{caller}: f_rest must be [{N}, Kr, 3]")
    widths = {(D + 1) ** 2 - 1: D for D in range(VP_SH_MAX_DEGREE + 1)}
    _require(int(f_rest.shape[1]) in widths,
             f"{caller}: f_rest has {int(f_rest.shape[1])} coefficient rows, not (D + 1)^2 - 1 for a degree D <= {VP_SH_MAX_DEGREE}")
    max_degree = widths[int(f_rest.shape[1])]
    _require(isinstance(degree, int) and 0 <= degree <= max_degree, f"{caller}: degree = {degree!r} outside [0, {max_degree}]")
    _require(f_rest.device == f_dc.device and means.device == f_dc.device, f"{caller}: f_dc, f_rest and means must be on one device")
    _require(N <= 2 ** 31 - 1, f"{caller}: N = {N} outside [0, 2^31 - 1]")
    return N, max_degree, f_dc.contiguous(), f_rest.contiguous(), means.contiguous()


def sh_colors(f_dc, f_rest, means, viewmat, degree, want_clamped=True):
    """vp_sh_colors: the colour rows f32 [N,3] of Gaussians with spherical-harmonics coefficients f_dc [N,3] and f_rest
    [N,Kr,3], seen from the camera of ``viewmat`` (host [4,4] world-to-camera; campos = -R^T t in float64), evaluated up to
    ``degree``: max(0.5 + sum_k Y_k(dir) sh[k], 0).  Returns (colors, clamped): clamped u8 [N] has bit c set where channel c
    was clamped (None without ``want_clamped``); sh_colors_backward needs it.  Asynchronous on the current stream."""
    import torch
    degree = int(degree)
    N, max_degree, f_dc, f_rest, means = _sh_inputs("sh_colors", f_dc, f_rest, means, degree)
    campos = (ctypes.c_float * 3)(*camera_position(viewmat))
    dev = f_dc.device
    colors = torch.empty((N, 3), dtype=torch.float32, device=dev)
    clamped = torch.empty(N, dtype=torch.uint8, device=dev) if want_clamped else None
    _call(dev, "vp_sh_colors", _ptr(f_dc), _ptr(f_rest), _ptr(means), campos, N, degree, max_degree, _ptr(colors), _ptr(clamped))
    return colors, clamped


def sh_colors_backward(f_dc, f_rest, means, viewmat, degree, grad_colors, clamped, *, want_dc=True, want_rest=True,
                       want_means=True, out_rest=None):
    """vp_sh_colors_backward: (grad_dc [N,3], grad_rest [N,Kr,3], grad_means [N,3]) of sh_colors for the upstream gradient
    grad_colors f32 [N,3] and the ``clamped`` bytes of the forward; None for an output not wanted.  grad_rest is written
    whole (zeros beyond the active degree), into ``out_rest`` when given.  Without ``want_means`` no coefficient is read."""
    import torch
    degree = int(degree)
    N, max_degree, f_dc, f_rest, means = _sh_inputs("sh_colors_backward", f_dc, f_rest, means, degree)
    dev = f_dc.device
    _require_tensors((grad_colors, "grad_colors", (torch.float32,)), (clamped, "clamped", (torch.uint8,)))
    _require(tuple(grad_colors.shape) == (N, 3) and tuple(clamped.shape) == (N,) and grad_colors.device == dev and
             clamped.device == dev, f"sh_colors_backward: grad_colors must be [{N}, 3] and clamped [{N}] on the coefficients' device")
    grad_colors, clamped = grad_colors.contiguous(), clamped.contiguous()
    campos = (ctypes.c_float * 3)(*camera_position(viewmat))
    grad_dc = torch.empty((N, 3), dtype=torch.float32, device=dev) if want_dc else None
    grad_means = torch.empty((N, 3), dtype=torch.float32, device=dev) if want_means else None
    grad_rest = None
    if want_rest:
        grad_rest = out_rest if out_rest is not None else torch.empty(tuple(f_rest.shape), dtype=torch.float32, device=dev)
        _require(isinstance(grad_rest, torch.Tensor) and grad_rest.is_cuda and grad_rest.device == dev and
                 grad_rest.dtype == torch.float32 and tuple(grad_rest.shape) == tuple(f_rest.shape) and grad_rest.is_contiguous(),
                 f"sh_colors_backward: out_rest must be a contiguous float32 CUDA tensor of shape {tuple(f_rest.shape)}")
    _call(dev, "vp_sh_colors_backward", _ptr(f_dc), _ptr(f_rest), _ptr(means), campos, N, degree, max_degree, _ptr(grad_colors),
          _ptr(clamped), _ptr(grad_dc), _ptr(grad_rest), _ptr(grad_means))
    return grad_dc, grad_rest, grad_means


VP_CODEBOOK_MAX_CODES = 256


def codebook_workspace_bytes(D, K, W, H):
    """vp_codebook_workspace_bytes: bytes of the workspace of codebook_assoc and codebook_loss for a D-channel W x H image
    and K codes (0 when out of range).  Needs no GPU."""
    return int(_entry("vp_codebook_workspace_bytes")(int(D), int(K), int(W), int(H)))


def _codebook_args(caller, image, ids, codebook, workspace):
    """The image f32 [D,H,W], the mask i32 [H,W] and the code book f32 [K,D], contiguous on one GPU, and the workspace."""
    import torch
    image, ids, _, D, H, W = _proto_maps(caller, image, ids, None)
    _require_tensors((codebook, "codebook", (torch.float32,)))
    _require(codebook.dim() == 2 and int(codebook.shape[1]) == D and codebook.device == image.device,
             f"{caller}: codebook must be float32 [K, {D}] on the image's device")
    K = int(codebook.shape[0])
    _require(1 <= K <= VP_CODEBOOK_MAX_CODES, f"K = {K} outside [1, {VP_CODEBOOK_MAX_CODES}]")
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(codebook_workspace_bytes(D, K, W, H), image.device)
    return image, ids, codebook.detach().contiguous(), D, H, W, K, ws, ptr


def codebook_assoc(image, ids, codebook, *, ignore_id=-1, want_pred=False, workspace=None):
    """vp_codebook_assoc: how much of every mask id's softmax mass falls on every code.  image f32 [D,H,W], ids int32 [H,W],
    codebook f32 [K,D] on one GPU.  Returns (score f64 [256,K], id_pixels int32 [256], pred int32 [H,W] or None, workspace);
    nothing is read back here."""
    import torch
    image, ids, codebook, D, H, W, K, ws, ptr = _codebook_args("codebook_assoc", image, ids, codebook, workspace)
    dev = image.device
    score = torch.empty((VP_PROTO_MAX_IDS, K), dtype=torch.float64, device=dev)
    id_pixels = torch.empty(VP_PROTO_MAX_IDS, dtype=torch.int32, device=dev)
    pred = torch.empty((H, W), dtype=torch.int32, device=dev) if want_pred else None
    _call(dev, "vp_codebook_assoc", image.data_ptr(), D, W, H, ids.data_ptr(), int(ignore_id), codebook.data_ptr(), K,
          score.data_ptr(), id_pixels.data_ptr(), _ptr(pred), ptr, ws.capacity())
    return score, id_pixels, pred, ws


def codebook_loss(image, ids, conf, codebook, assign, *, conf_min=0.2, ignore_id=-1, want_pixel_loss=False, workspace=None):
    """vp_codebook_loss: cross-entropy and clustering loss of the code book against the labels ``assign`` (int32 [256] on
    the device: id -> code, -1 = takes no part) gives every pixel, over the pixels ``conf`` (f32 [H,W] or None) accepts.
    Returns (stats f64 [4] = {sum of cross-entropy terms, sum of |s - B_v|, participating pixels, mismatched pixels},
    grad_cls f32 [K,D], grad_cluster f32 [K,D], pixel_loss f32 [H,W] or None, workspace); nothing is read back here."""
    import torch
    image, ids, codebook, D, H, W, K, ws, ptr = _codebook_args("codebook_loss", image, ids, codebook, workspace)
    dev = image.device
    (conf,) = _splat_images(dev, (conf, "conf", (H, W), torch.float32))
    _require_tensors((assign, "assign", (torch.int32,)))
    _require(tuple(assign.shape) == (VP_PROTO_MAX_IDS,) and assign.device == dev,
             f"assign must be int32 [{VP_PROTO_MAX_IDS}] on the image's device")
    assign = assign.contiguous()
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    grad_cls = torch.empty((K, D), dtype=torch.float32, device=dev)
    grad_cluster = torch.empty((K, D), dtype=torch.float32, device=dev)
    pixel_loss = torch.empty((H, W), dtype=torch.float32, device=dev) if want_pixel_loss else None
    _call(dev, "vp_codebook_loss", image.data_ptr(), D, W, H, ids.data_ptr(), int(ignore_id), _ptr(conf), float(conf_min),
          codebook.data_ptr(), K, assign.data_ptr(), stats.data_ptr(), grad_cls.data_ptr(), grad_cluster.data_ptr(),
          _ptr(pixel_loss), ptr, ws.capacity())
    return stats, grad_cls, grad_cluster, pixel_loss, ws


VP_KNN_MAX_K = 15
VP_NEIGHBOR_KL_MAX_P = 256
VP_NEIGHBOR_KL_MAX_K = 16


def knn_points(points, k, queries=None, *, cell_order=True, want_d2=True):
    """vp_knn_points: the k nearest OTHER points of every query among ``points`` (f32 [N,3] on a GPU), exact, ordered by
    (squared distance in float64, index).  ``queries`` None: the points themselves, each one left out of its own result.
    Returns (idx int32 [M,k], d2 float64 [M,k] or None) on the device; -1 / +inf where fewer than k other points exist.
    ``cell_order`` (self-queries only): launch the queries in the grid's cell order, so that a wavefront's lanes walk the
    same cells, and put the rows back in torch; False launches them in the caller's order (the same result)."""
    import torch
    import voxel_to_gaussian_map
    _require_tensors((points, "points", (torch.float32,)))
    _require(points.dim() == 2 and int(points.shape[1]) == 3 and points.is_cuda, "points must be float32 [N, 3] on a GPU")
    _require(1 <= int(k) <= VP_KNN_MAX_K, f"k = {k} outside [1, {VP_KNN_MAX_K}]")
    dev = points.device
    N, k = int(points.shape[0]), int(k)
    _require(N >= 1, "points is empty")
    pts, perm, start, origin, h, dims = voxel_to_gaussian_map._bucket(points.detach(), dev)
    self_index = None
    if queries is None:
        q, self_index = (pts, perm) if cell_order else (points.detach().contiguous(), torch.arange(N, dtype=torch.int32, device=dev))
    else:
        _require_tensors((queries, "queries", (torch.float32,)))
        _require(queries.dim() == 2 and int(queries.shape[1]) == 3 and queries.device == dev,
                 "queries must be float32 [M, 3] on the points' device")
        q = queries.detach().contiguous()
    M = int(q.shape[0])
    idx = torch.empty((M, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((M, k), dtype=torch.float64, device=dev) if want_d2 else None
    g = (ctypes.c_double * 3)(*origin)
    _call(dev, "vp_knn_points", pts.data_ptr(), perm.data_ptr(), start.data_ptr(), g, ctypes.c_double(h), dims[0], dims[1],
          dims[2], q.data_ptr(), _ptr(self_index), M, k, idx.data_ptr(), _ptr(d2))
    if queries is None and cell_order:       # row t of the launch is point perm[t]
        back = perm.long()
        idx = torch.empty_like(idx).index_copy_(0, back, idx)
        d2 = torch.empty_like(d2).index_copy_(0, back, d2) if d2 is not None else None
    return idx, d2


def knn_mean_dist2(points):
    """The counterpart of simple-knn's distCUDA2 (submodules/simple-knn/simple_knn.cu:132-182, read by
    scene/gaussian_model.py:150): per point the mean of the three smallest squared distances to other points, float32 [N].
    The three distances are vp_knn_points' float64 ones, their mean (d0 + d1) + d2 over 3 is taken in float64 and rounded once; a point with fewer
    than three others takes the mean over those it has (0 for a lone point)."""
    import torch
    _, d2 = knn_points(points, 3)
    have = torch.isfinite(d2)
    z = torch.where(have, d2, torch.zeros_like(d2))
    return (((z[:, 0] + z[:, 1]) + z[:, 2]) / have.sum(1).clamp_min(1)).to(torch.float32)


def _rows3(t, name, dev=None):
    """``t`` as a contiguous float32 [M,3] on a GPU (on ``dev`` when given)."""
    import torch
    _require_tensors((t, name, (torch.float32,)))
    _require(t.dim() == 2 and int(t.shape[1]) == 3 and (dev is None or t.device == dev),
             f"{name} must be float32 [M, 3]" + (" on the points' device" if dev is not None else ""))
    return t.detach().contiguous()


def ball_count(points, radius_or_radii, queries=None, normals=None, query_normals=None, min_dot=None):
    """vp_ball_count (the contract is in include/voxproj_grid.h): per query the number of ``points`` (f32 [N,3] on a GPU)
    with float64 squared distance <= r^2, boundary points and the query itself included, as cKDTree.query_ball_point counts
    them.  ``radius_or_radii``: a Python float, or a float32 [M] tensor with one radius per query.  ``queries`` None: the
    points themselves.  With ``normals`` (unit, f32 [N,3]; ``query_normals`` f32 [M,3] for queries that are not the points)
    and ``min_dot`` also the number of points within the ball whose normal has a float64 dot product > min_dot with the
    query's.  Returns (count int32 [M], consistent int32 [M] or None) on the device, in the caller's row order.  The points'
    bounds (and the largest radius of a radii tensor) are read back to lay out the grid before the kernel is launched, as
    knn_points does: the call synchronises the current stream once; the counts themselves are not read back.  The queries
    are launched in the grid's cell order, so that a wavefront's lanes walk the same cells."""
    import torch
    import voxel_to_gaussian_map
    points = _rows3(points, "points")
    dev, N = points.device, int(points.shape[0])
    q = points if queries is None else _rows3(queries, "queries", dev)
    M = int(q.shape[0])
    radii = None
    if isinstance(radius_or_radii, torch.Tensor):
        _require_tensors((radius_or_radii, "radii", (torch.float32,)))
        _require(tuple(radius_or_radii.shape) == (M,) and radius_or_radii.device == dev, f"radii must be float32 [{M}] on the points' device")
        radii, radius = radius_or_radii.detach().contiguous(), 0.0
    else:
        radius = float(radius_or_radii)
        _require(0.0 <= radius < float("inf"), f"radius = {radius} must be finite and >= 0")
    _require((normals is None) == (min_dot is None), "normals and min_dot go together")
    qn = None
    if normals is not None:
        normals = _rows3(normals, "normals", dev)
        _require(int(normals.shape[0]) == N, f"normals must be [{N}, 3]")
        _require(queries is None or query_normals is not None, "queries that are not the points need query_normals")
        qn = normals if queries is None else _rows3(query_normals, "query_normals", dev)
        _require(int(qn.shape[0]) == M, f"query_normals must be [{M}, 3]")
    else:
        _require(query_normals is None, "query_normals without normals")
    count = torch.zeros(M, dtype=torch.int32, device=dev)
    consistent = torch.zeros(M, dtype=torch.int32, device=dev) if normals is not None else None
    if N == 0 or M == 0:
        return count, consistent
    # cells no smaller than the largest finite radius: the box of a query is 3 x 3 x 3 cells
    if radii is not None:
        finite = radii[torch.isfinite(radii)].abs()
        rmax = float(finite.max()) if finite.numel() else 0.0
    else:
        rmax = radius
    pts, perm, start, origin, h, dims = voxel_to_gaussian_map._bucket(points, dev, min_cell=rmax if rmax > 0.0 else None)
    if queries is None:
        order = perm.long()
        qs = pts
    else:                                        # the queries in the order of the cell nearest to them
        lo = torch.tensor(origin, dtype=torch.float64, device=dev)
        cell = torch.floor((q.double() - lo) / h).nan_to_num(nan=0.0).clamp(-1.0, 2.0 ** 31)
        for a in range(3):
            cell[:, a].clamp_(0, dims[a] - 1)
        cell = cell.long()
        order = torch.argsort((cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0], stable=True)
        qs = q[order].contiguous()
    rs = radii[order].contiguous() if radii is not None else None
    qns = qn[order].contiguous() if qn is not None else None
    cnt = torch.empty(M, dtype=torch.int32, device=dev)
    con = torch.empty(M, dtype=torch.int32, device=dev) if normals is not None else None
    g = (ctypes.c_double * 3)(*origin)
    _call(dev, "vp_ball_count", pts.data_ptr(), perm.data_ptr(), start.data_ptr(), g, ctypes.c_double(h), dims[0], dims[1],
          dims[2], qs.data_ptr(), M, ctypes.c_double(radius), _ptr(rs), _ptr(normals), _ptr(qns),
          ctypes.c_double(float(min_dot) if min_dot is not None else 0.0), cnt.data_ptr(), _ptr(con))
    count.index_copy_(0, order, cnt)                 # row t of the launch is query order[t]
    if con is not None:
        consistent.index_copy_(0, order, con)
    return count, consistent


def voxel_grid_workspace_bytes(N):
    nbytes = int(_entry("vp_voxel_grid_workspace_bytes")(int(N)))
    _require(nbytes > 0, f"no workspace size for N = {N}")
    return nbytes


def voxel_grid(points, colors, voxel_size, keep=None, workspace=None):
    """vp_voxel_grid (the contract is in include/voxproj_grid.h): the sparse voxel grid of the kept ``points`` (f32 [N,3] on a
    GPU) with ``colors`` uint8 [N,3]; ``keep`` uint8 or bool [N] or None (all).  Returns dict(centers f32 [V,3], colors uint8
    [V,3], counts int32 [V], voxel_index int32 [V,3], point_voxel int32 [N] (-1: not kept), n_voxels int32 [1], min_corner
    f32 [3], status int32 [1]) on the device, the voxels in lexicographic (x, y, z) order.  The 4-byte voxel count is read
    once to trim the rows, as mesh_render reads its pair count.  status 1 (a non-finite kept point, or a cell index above
    2^21 - 1): no voxel, V = 0; the caller decides what that means.  ``workspace``: a SplatWorkspace, kept across calls."""
    import torch
    points = _rows3(points, "points")
    dev, N = points.device, int(points.shape[0])
    _require_tensors((colors, "colors", (torch.uint8,)))
    _require(tuple(colors.shape) == (N, 3) and colors.device == dev, f"colors must be uint8 [{N}, 3] on the points' device")
    colors = colors.contiguous()
    if keep is not None:
        _require_tensors((keep, "keep", (torch.uint8, torch.bool)))
        _require(tuple(keep.shape) == (N,) and keep.device == dev, f"keep must be uint8 or bool [{N}] on the points' device")
        keep = keep.to(torch.uint8).contiguous()
    vs = float(voxel_size)
    _require(0.0 < vs < float("inf"), f"voxel_size = {voxel_size} must be finite and > 0")
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(voxel_grid_workspace_bytes(N), dev)
    centers = torch.empty((N, 3), dtype=torch.float32, device=dev)
    vcolors = torch.empty((N, 3), dtype=torch.uint8, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    vindex = torch.empty((N, 3), dtype=torch.int32, device=dev)
    point_voxel = torch.full((N,), -1, dtype=torch.int32, device=dev)
    n_voxels = torch.zeros(1, dtype=torch.int32, device=dev)
    min_corner = torch.full((3,), float("inf"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _call(dev, "vp_voxel_grid", _ptr(points), _ptr(colors), _ptr(keep), N, ctypes.c_double(vs), _ptr(centers), _ptr(vcolors),
          _ptr(counts), _ptr(vindex), _ptr(point_voxel), n_voxels.data_ptr(), min_corner.data_ptr(), status.data_ptr(), ptr,
          ws.capacity())
    V = int(n_voxels.item())
    return dict(centers=centers[:V], colors=vcolors[:V], counts=counts[:V], voxel_index=vindex[:V], point_voxel=point_voxel,
                n_voxels=n_voxels, min_corner=min_corner, status=status)


def _feature_rows(rows, caller):
    """The [N, C] table of the label-sum calls: float16 or float32 on a GPU, unit channel stride, row stride >= C."""
    import torch
    _require_tensors((rows, "rows", (torch.float16, torch.float32)))
    _require(rows.dim() == 2 and rows.shape[1] > 0, f"{caller}: rows must be [N, C] with C >= 1")
    _require(int(rows.shape[1]) <= 4096, f"{caller}: C = {int(rows.shape[1])} must be in [1, 4096]")
    if rows.shape[0] > 1 and (rows.stride(1) != 1 or rows.stride(0) < rows.shape[1]):
        rows = rows.contiguous()
    stride = int(rows.stride(0)) if rows.shape[0] > 1 else int(rows.shape[1])
    return rows, int(rows.shape[0]), int(rows.shape[1]), stride


def row_inv_norms(rows, check=False):
    """vp_row_inv_norms (the contract is in include/voxproj_cluster.h): (inv float32 [N], status int32 [2]) on the rows' device,
    inv[r] = 1 / max(|rows[r]|, 1e-12) with the norm in float64; an all-zero row gets 0 and is counted in status[0], a row with a
    non-finite element gets 0 and is counted in status[1].  Asynchronous on the current stream, except with ``check``: then the
    call synchronises and raises VoxprojError if any row was zero or non-finite."""
    import torch
    rows, N, C, stride = _feature_rows(rows, "row_inv_norms")
    dev = rows.device
    inv = torch.empty(N, dtype=torch.float32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    _call(dev, "vp_row_inv_norms", _ptr(rows) if N else None, int(rows.dtype == torch.float16), N, C, stride, _ptr(inv) if N else None,
          status.data_ptr())
    if check:
        zero, bad = (int(v) for v in status.tolist())
        if zero or bad:
            raise VoxprojError(f"row_inv_norms: {zero} all-zero row(s) and {bad} row(s) with a non-finite element (inverse norm 0)")
    return inv, status


def _label_sums_part_rows(n_rows, part_rows):
    """cl_part_rows (csrc/vp_cluster.h): a given R is capped by the table's length, the default R is not."""
    return min(int(part_rows), max(int(n_rows), 1)) if part_rows else max(256, -(-int(n_rows) // 32768))


def label_sums_workspace_bytes(n_rows, K, C, part_rows=0):
    """vp_label_sums_workspace_bytes, plus the room the partial rows of a ``part_rows`` below the default take (the rule is in
    include/voxproj_cluster.h)."""
    n_rows, K, C = int(n_rows), int(K), int(C)
    nbytes = int(_entry("vp_label_sums_workspace_bytes")(n_rows, K, C))
    _require(nbytes > 0, f"no workspace size for n_rows = {n_rows}, K = {K}, C = {C}")
    # (the default R of a table of fewer than 256 rows is longer than the table: capping it too counted one default part too
    # many, and a call with part_rows on such a table was refused wherever C * 4 bytes exceed the slack of the other sections)
    parts = [min(n_rows, n_rows // R + min(K, n_rows))
             for R in (_label_sums_part_rows(n_rows, part_rows), _label_sums_part_rows(n_rows, 0))]
    return nbytes + (-(-max(parts[0] - parts[1], 0) * C * 4 // 256)) * 256


def label_sums(rows, labels, K, row_scale=None, part_rows=0, check=True, workspace=None):
    """vp_label_sums (the contract is in include/voxproj_cluster.h): sums[k] = the sum of row_scale[r] * rows[r] over the rows
    with labels[r] == k, in a fixed order, without float atomics.  rows float16 or float32 [N, C] on a GPU (any row stride),
    labels int32 [N], row_scale float32 [N] or None (1), 1 <= K <= 65536.  Returns (sums float32 [K, C], counts int32 [K],
    status int32 [2]: rows with label < 0 (ignored), rows with label >= K (left out as well)) on the device.  Asynchronous on
    the current stream, except with ``check``: then the call synchronises and raises VoxprojError if a label was >= K.
    ``workspace``: a SplatWorkspace, kept across calls."""
    import torch
    rows, N, C, stride = _feature_rows(rows, "label_sums")
    dev = rows.device
    K, part_rows = int(K), int(part_rows)
    _require(1 <= K <= 65536, f"K = {K} must be in [1, 65536]")
    _require(part_rows >= 0, f"part_rows = {part_rows} must be >= 0 (0 = the default)")
    _require_tensors((labels, "labels", (torch.int32,)))
    _require(tuple(labels.shape) == (N,) and labels.device == dev, f"labels must be int32 [{N}] on the rows' device")
    labels = labels.contiguous()
    if row_scale is not None:
        _require_tensors((row_scale, "row_scale", (torch.float32,)))
        _require(tuple(row_scale.shape) == (N,) and row_scale.device == dev, f"row_scale must be float32 [{N}] on the rows' device")
        row_scale = row_scale.contiguous()
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(label_sums_workspace_bytes(N, K, C, part_rows), dev)
    sums = torch.empty((K, C), dtype=torch.float32, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    _call(dev, "vp_label_sums", _ptr(rows) if N else None, int(rows.dtype == torch.float16), N, C, stride, _ptr(labels) if N else None,
          _ptr(row_scale), K, part_rows, sums.data_ptr(), counts.data_ptr(), status.data_ptr(), ptr, ws.capacity())
    if check:
        over = int(status[1].item())
        if over:
            raise VoxprojError(f"label_sums: {over} row(s) carry a label >= K = {K} (left out of every sum)")
    return sums, counts, status


def reverse_table(nbr, n_rows):
    """The reversed form of a neighbour table ``nbr`` int [S, k-1] (entries in [0, n_rows), anything else = none), CSR over
    rows: (rev_start int32 [n_rows+1], rev_entry int32 [S (k-1)]).  rev_entry[rev_start[i] : rev_start[i+1]] are the flat
    entries s (k-1) + j that name row i, ascending (a stable sort); entries that name no row sit behind rev_start[n_rows]."""
    import torch
    flat = nbr.reshape(-1).long()
    key = torch.where((flat >= 0) & (flat < n_rows), flat, torch.full_like(flat, n_rows))
    order = torch.argsort(key, stable=True)
    start = torch.zeros(n_rows + 1, dtype=torch.int32, device=nbr.device)
    start[1:] = torch.cumsum(torch.bincount(key, minlength=n_rows + 1)[:n_rows], 0).to(torch.int32)
    return start, order.to(torch.int32).contiguous()


class NeighborSample:
    """What one application of the regulariser reads: the sample list (None: every row in order), its rows of the neighbour
    table, and both reversed tables; built by NeighborTable.all / .select."""

    def __init__(self, n_rows, k, samples, nbr):
        import torch
        self.n_rows, self.k = int(n_rows), int(k)
        self.samples = None if samples is None else samples.to(torch.int32).contiguous()
        self.nbr = nbr.contiguous()
        self.S = int(self.nbr.shape[0])
        self.rev_start, self.rev_entry = reverse_table(self.nbr, self.n_rows)
        self.smp_start = self.smp_entry = None
        if self.samples is not None:
            self.smp_start, self.smp_entry = reverse_table(self.samples.reshape(-1, 1), self.n_rows)
            if self.S == 0:              # an empty list is still a list: a non-NULL pointer that is never read
                self.samples = torch.zeros(1, dtype=torch.int32, device=self.nbr.device)


class NeighborTable:
    """The neighbour table of the regulariser, built once from the points (f32 [N,3] on a GPU): ``nbr`` int32 [N, k-1], the
    k - 1 nearest other points of every point (k counts the point itself, like the reference's reg3d_k), and its reversed
    form, both on the device."""

    def __init__(self, points, k):
        _require(2 <= int(k) <= VP_NEIGHBOR_KL_MAX_K, f"k = {k} outside [2, {VP_NEIGHBOR_KL_MAX_K}] (k counts the point itself)")
        self.k = int(k)
        self.n_rows = int(points.shape[0])
        self.nbr, _ = knn_points(points, self.k - 1, want_d2=False)
        self.all = NeighborSample(self.n_rows, self.k, None, self.nbr)
        self.rev_start, self.rev_entry = self.all.rev_start, self.all.rev_entry

    def select(self, samples):
        """The tables of one sample list (integer tensor [S] of rows in [0, N), repeats allowed) on the table's device."""
        samples = samples.to(self.nbr.device)
        return NeighborSample(self.n_rows, self.k, samples, self.nbr[samples.long()])


def neighbor_kl_workspace_bytes(S):
    """vp_neighbor_kl_workspace_bytes: bytes of neighbor_kl's workspace for S sample positions.  Needs no GPU."""
    return int(_entry("vp_neighbor_kl_workspace_bytes")(int(S)))


def _neighbor_kl_logits(logits):
    import torch
    _require_tensors((logits, "logits", (torch.float32,)))
    _require(logits.dim() == 2 and logits.is_cuda, "logits must be float32 [N, P] on a GPU")
    N, P = int(logits.shape[0]), int(logits.shape[1])
    _require(N >= 1 and 1 <= P <= VP_NEIGHBOR_KL_MAX_P, f"logits [{N}, {P}]: N >= 1 and P in [1, {VP_NEIGHBOR_KL_MAX_P}]")
    logits = logits.detach()
    if logits.stride(1) != 1 or logits.stride(0) < P:
        logits = logits.contiguous()
    return logits, N, P


def neighbor_kl(logits, sample, *, want_sample_loss=False, lanes=0, workspace=None):
    """vp_neighbor_kl: the neighbourhood KL sum of ``logits`` (f32 [N,P], unit channel stride) over a NeighborSample.
    Returns (stats f64 [2] = {sum, S}, row_lse f32 [N], sample_loss f32 [S] or None, workspace) on the device; the loss is
    scale / (S k P) stats[0].  Nothing is read back here."""
    import torch
    logits, N, P = _neighbor_kl_logits(logits)
    _require(sample.n_rows == N and sample.nbr.device == logits.device, "the neighbour table is of another point set or device")
    dev = logits.device
    ws = workspace if workspace is not None else SplatWorkspace()
    ptr = ws.ensure(neighbor_kl_workspace_bytes(sample.S), dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    row_lse = torch.empty(N, dtype=torch.float32, device=dev)
    sample_loss = torch.empty(sample.S, dtype=torch.float32, device=dev) if want_sample_loss else None
    _call(dev, "vp_neighbor_kl", logits.data_ptr(), N, P, logits.stride(0), _ptr(sample.samples), sample.S, _ptr(sample.nbr),
          sample.k, row_lse.data_ptr(), _ptr(sample_loss), stats.data_ptr(), int(lanes), ptr, ws.capacity())
    return stats, row_lse, sample_loss, ws


def neighbor_kl_gradient(logits, sample, row_lse, *, scale=2.0, grad_loss=None, lanes=0, out=None):
    """vp_neighbor_kl_gradient: the gradient of scale / (S k P) stats[0] with respect to the logits, times ``grad_loss``
    (f32 one element on the device, or None): f32 [N,P], every row written.  ``row_lse`` is neighbor_kl's, of the same logits."""
    import torch
    logits, N, P = _neighbor_kl_logits(logits)
    _require(sample.n_rows == N and sample.nbr.device == logits.device, "the neighbour table is of another point set or device")
    dev = logits.device
    _require_tensors((row_lse, "row_lse", (torch.float32,)))
    _require(tuple(row_lse.shape) == (N,) and row_lse.device == dev and row_lse.is_contiguous(), f"row_lse must be float32 [{N}]")
    (grad_loss,) = _splat_images(dev, (grad_loss, "grad_loss", None, torch.float32))
    if out is None:
        out = torch.empty((N, P), dtype=torch.float32, device=dev)
    _require(out.dtype == torch.float32 and tuple(out.shape) == (N, P) and out.device == dev and out.stride(1) == 1 and
             out.stride(0) >= P, f"out must be float32 [{N}, {P}] with a unit channel stride")
    _call(dev, "vp_neighbor_kl_gradient", logits.data_ptr(), N, P, logits.stride(0), _ptr(sample.samples), sample.S,
          _ptr(sample.nbr), sample.k, row_lse.data_ptr(), sample.rev_start.data_ptr(), _ptr(sample.rev_entry),
          _ptr(sample.smp_start), _ptr(sample.smp_entry), float(scale), _ptr(grad_loss), out.data_ptr(), out.stride(0),
          int(lanes))
    return out


def assign_view_ids(score, id_pixels, K):
    """The linear assignment of one view's mask ids to the codes ("virtual labels"), on the host.  score [256,K] and
    id_pixels [256] are codebook_assoc's outputs (tensors or arrays).  Labels are the ids with id_pixels > 0 in ascending
    order, the first K of them when there are more; scipy.optimize.linear_sum_assignment maximises the assigned score.
    Returns a numpy int32 [256]: the code of every label, -1 elsewhere.  With device tensors this is one small
    device-to-host copy and one host synchronisation per view, as in the method this follows."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    score = np.asarray(score.detach().cpu() if hasattr(score, "detach") else score, dtype=np.float64)
    id_pixels = np.asarray(id_pixels.detach().cpu() if hasattr(id_pixels, "detach") else id_pixels)
    K = int(K)
    _require(score.shape == (VP_PROTO_MAX_IDS, K) and id_pixels.shape == (VP_PROTO_MAX_IDS,),
             f"score must be [{VP_PROTO_MAX_IDS}, {K}] and id_pixels [{VP_PROTO_MAX_IDS}]")
    labels = np.flatnonzero(id_pixels > 0)[:K]
    out = np.full(VP_PROTO_MAX_IDS, -1, np.int32)
    if len(labels):
        rows, cols = linear_sum_assignment(-score[labels])
        out[labels[rows]] = cols.astype(np.int32)
    return out


class LabelScores:
    """The four device tensors vp_label_scores accumulates into: confusion i64 [P,P] (rows = ground truth), skipped i64 [2]
    ({target not valid, target valid under a prediction that is not}), bnd_inter and bnd_union i64 [P]."""

    def __init__(self, P, device):
        import torch
        _require(1 <= int(P) <= 256, f"P = {P} outside [1, 256]")
        self.P = int(P)
        self.confusion = torch.zeros(self.P, self.P, dtype=torch.int64, device=device)
        self.skipped = torch.zeros(2, dtype=torch.int64, device=device)
        self.bnd_inter = torch.zeros(self.P, dtype=torch.int64, device=device)
        self.bnd_union = torch.zeros(self.P, dtype=torch.int64, device=device)

    def zero_(self):
        for t in (self.confusion, self.skipped, self.bnd_inter, self.bnd_union):
            t.zero_()
        return self

    def numpy(self):
        """(confusion, skipped, bnd_inter, bnd_union) as numpy int64 arrays (one synchronising download each)."""
        return tuple(t.cpu().numpy() for t in (self.confusion, self.skipped, self.bnd_inter, self.bnd_union))


def _label_map(t, name, dev=None, shape=None):
    """A [H,W] CUDA tensor of any integer dtype as contiguous int32 (the conversion is plumbing; int32 passes untouched).
    An int64 value outside int32 becomes -1: a label that is not valid, instead of wrapping into a class."""
    import torch
    _require(isinstance(t, torch.Tensor) and t.is_cuda, f"{name} must be a CUDA tensor")
    _require(not t.dtype.is_floating_point and not t.dtype.is_complex and t.dtype != torch.bool,
             f"{name} must have an integer dtype, not {t.dtype}")
    _require(t.dim() == 2 and t.numel() > 0, f"{name} must be [H, W]")
    _require(dev is None or t.device == dev, f"{name} must be on the other map's device")
    _require(shape is None or tuple(t.shape) == tuple(shape), f"{name} must be {list(shape) if shape else ''} like the other map")
    if t.dtype == torch.int64:
        t = torch.where((t < -(1 << 31)) | (t >= (1 << 31)), torch.full_like(t, -1), t)
    return t.to(torch.int32).contiguous()


def _label_workspace(workspace, W, H, dev):
    ws = workspace if workspace is not None else SplatWorkspace()
    nbytes = int(lib().vp_label_scores_workspace_bytes(int(W), int(H)))
    _require(nbytes > 0, f"image size {W} x {H} outside [1, 32768]")
    return ws, ws.ensure(nbytes, dev)


def label_boundary(labels, radius, workspace=None):
    """vp_label_boundary: the u8 [H,W] boundary band of an integer label map for ``radius`` in [1, 4096] (1 where the
    (2 radius + 1)^2 window leaves the image or holds another label).  ``workspace``: a SplatWorkspace to reuse."""
    import torch
    labels = _label_map(labels, "labels")
    H, W = (int(v) for v in labels.shape)
    dev = labels.device
    ws, ptr = _label_workspace(workspace, W, H, dev)
    band = torch.empty((H, W), dtype=torch.uint8, device=dev)
    _call(dev, "vp_label_boundary", labels.data_ptr(), W, H, int(radius), band.data_ptr(), ptr, ws.capacity())
    return band


def label_scores(pred, target, P, radius=0, out=None, workspace=None):
    """vp_label_scores: add one view to ``out`` (a LabelScores; a fresh, zeroed one when None) and return it.  pred, target:
    CUDA tensors [H,W] of any integer dtype (int64 values outside int32 count as -1); a label is valid when 0 <= v < P.
    radius = 0: confusion and skipped only;
    radius > 0: the boundary counts too, through ``workspace`` (a SplatWorkspace, reused and grown as splat_loss does; a
    fresh one when None).  Nothing is read back here."""
    pred = _label_map(pred, "pred")
    target = _label_map(target, "target", pred.device, pred.shape)
    H, W = (int(v) for v in pred.shape)
    dev = pred.device
    if out is None:
        out = LabelScores(P, dev)
    _require(isinstance(out, LabelScores) and out.P == int(P) and out.confusion.device == dev,
             f"out must be a LabelScores of {P} classes on the maps' device")
    radius = int(radius)
    ws, ptr = (None, None)
    if radius > 0:
        ws, ptr = _label_workspace(workspace, W, H, dev)
    _call(dev, "vp_label_scores", pred.data_ptr(), target.data_ptr(), W, H, int(P), radius, out.confusion.data_ptr(),
          out.skipped.data_ptr(), out.bnd_inter.data_ptr() if radius > 0 else None,
          out.bnd_union.data_ptr() if radius > 0 else None, ptr, ws.capacity() if ws is not None else 0)
    return out


def counters(ws, device):
    """Device-side diagnostic counters of the last call: dict(bad_id, box_miss, n_heavy, heavy_t, n_parts, n_split) -- n_heavy = voxels
    above the heavy threshold in force (heavy_t: the option or min(256 + 64*B*V, 2048), raised to the part-slot bound where that binds;
    one-view calls: the device's choice, see below), n_split = the voxels cut into parts, n_parts = their parts; part_t / part_px =
    pixels above which a voxel was cut and pixels per part; n_hit = pixels whose ray hit a voxel (counted only by one-view calls
    that size their parts from it: part_px = max(32, 2 * n_hit / slots), part_t = heavy_t = 2 * part_px)."""
    import torch
    arr = (ctypes.c_int32 * 32)()
    ptr = ws.ptr()
    stream = torch.cuda.current_stream(device).cuda_stream
    check(lib().vp_workspace_counters(ptr, arr, 32, stream))
    return dict(bad_id=int(arr[0]), box_miss=int(arr[1]), n_heavy=int(arr[2]), heavy_t=int(arr[7]), n_parts=int(arr[24]), n_split=int(arr[25]),
                n_hit=int(arr[8]), part_t=int(arr[9]), part_px=int(arr[10]))


def table_builds(ws):
    """How many times the occupancy-derived tables of workspace ``ws`` have been built (diagnostic)."""
    return int(lib().vp_workspace_table_builds(ws.ptr()))


def profile_enable(on=True):
    check(lib().vp_profile_enable(1 if on else 0))


def profile_read():
    """Summed HIP-event milliseconds and launch counts per kernel group since the last read."""
    ms = (ctypes.c_double * 4)()
    n = (ctypes.c_int64 * 4)()
    check(lib().vp_profile_read(ms, n))
    return dict(prep_ms=ms[0], first_hit_ms=ms[1], gather_ms=ms[2], heavy_ms=ms[3],
                prep_launches=int(n[0]), first_hit_launches=int(n[1]), gather_launches=int(n[2]),
                heavy_launches=int(n[3]))


def workspace_status(ws, device):
    """Synchronise and raise if any call on ``ws`` reported a device-side error (asynchronous callers)."""
    import torch
    stream = torch.cuda.current_stream(device).cuda_stream
    check(lib().vp_workspace_status(ws.ptr(), stream))


def project_colors_raw(occ_zyx, c2w, intr, grid_origin3, voxel_size, images, color_sum, hit_count, first_view=None,
                       view_base=0, pixel_uv=None):
    """vp_project_colors on torch CUDA tensors: occ i32 [Z,Y,X], c2w f32 [V,4,4], intr f32 [V,4],
    images u8 [V,H,W,3]; color_sum f32 [n_rows,3], hit_count i32 [n_rows], first_view i32 [n_rows] or None,
    pixel_uv i32 [V,n_rows,2] or None (receives the sampled pixel per view and voxel ID, -1 where unseen)."""
    import torch
    dev = occ_zyx.device
    assert occ_zyx.is_cuda and occ_zyx.dtype == torch.int32 and occ_zyx.is_contiguous()
    V = int(images.shape[0])
    assert images.dtype == torch.uint8 and images.is_contiguous() and images.shape[-1] == 3
    assert c2w.dtype == torch.float32 and c2w.is_contiguous() and c2w.numel() == V * 16
    assert intr.dtype == torch.float32 and intr.is_contiguous() and intr.numel() == V * 4
    assert color_sum.dtype == torch.float32 and color_sum.is_contiguous() and hit_count.dtype == torch.int32
    n_rows = int(hit_count.shape[0])
    if pixel_uv is not None:
        assert pixel_uv.dtype == torch.int32 and pixel_uv.is_contiguous() and tuple(pixel_uv.shape) == (V, n_rows, 2)
    need = int(lib().vp_colors_workspace_bytes(n_rows))
    scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ptr = (scratch.data_ptr() + 255) & ~255
    g = (ctypes.c_float * 3)(*[float(v) for v in grid_origin3])
    Z, Y, X = occ_zyx.shape
    _call(dev, "vp_project_colors", occ_zyx.data_ptr(), Z, Y, X, c2w.data_ptr(), intr.data_ptr(), V, g,
          ctypes.c_double(float(voxel_size)), images.data_ptr(), int(images.shape[1]), int(images.shape[2]), color_sum.data_ptr(),
          hit_count.data_ptr(), first_view.data_ptr() if first_view is not None else None,
          pixel_uv.data_ptr() if pixel_uv is not None else None, n_rows, int(view_base), ptr, need)


def upsample_features(src_chw, H, W, keep_dtype=False, out=None):
    """vp_upsample_features: CUDA tensor [C,h,w] (float16 or float32) -> channels-last [H,W,C], float32 or (float16
    source with ``keep_dtype``) float16.  The counterpart of prepare_tensor_data.py:119-127,152,183-185; asynchronous on
    the current stream.  ``out``: optional destination tensor (e.g. a slot of a resident pool)."""
    import torch
    assert src_chw.is_cuda and src_chw.dim() == 3 and src_chw.dtype in (torch.float16, torch.float32)
    src = src_chw.contiguous()
    C, h, w = (int(v) for v in src.shape)
    src16 = src.dtype == torch.float16
    dst_dtype = torch.float16 if (keep_dtype and src16) else torch.float32
    if out is None:
        out = torch.empty((H, W, C), dtype=dst_dtype, device=src.device)
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (H, W, C) and out.dtype == dst_dtype
    need = int(lib().vp_upsample_workspace_bytes(C, h, w, int(src16)))
    scratch = torch.empty(need + 256, dtype=torch.uint8, device=src.device)
    ptr = (scratch.data_ptr() + 255) & ~255
    _call(src.device, "vp_upsample_features", src.data_ptr(), int(src16), C, h, w, out.data_ptr(),
          int(dst_dtype == torch.float16), int(H), int(W), ptr, need)
    return out


def build_occupancy_device(points_xyz, grid_origin3, voxel_size):
    """vp_voxel_coords + vp_scatter_occupancy: CUDA float32 [N,3] points -> (occ int32 [Z,Y,X] on the same device,
    min_coord int[3] before the shift).  build_sparse_occupancy.py:30-53: half-to-even rounding in float32, the grid is
    shifted to start at zero when any coordinate is negative, the last vertex wins on duplicates."""
    import torch
    assert points_xyz.is_cuda and points_xyz.dtype == torch.float32 and points_xyz.dim() == 2 and points_xyz.shape[1] == 3
    pts = points_xyz.contiguous()
    N = int(pts.shape[0])
    dev = pts.device
    coords = torch.empty((N, 3), dtype=torch.int32, device=dev)
    scratch = torch.zeros(8, dtype=torch.int32, device=dev)
    mm = (ctypes.c_int32 * 6)()
    g = (ctypes.c_float * 3)(*[float(v) for v in grid_origin3])
    _call(dev, "vp_voxel_coords", pts.data_ptr(), N, g, ctypes.c_float(float(voxel_size)), coords.data_ptr(), scratch.data_ptr(), mm)
    lo, hi = [int(mm[k]) for k in range(3)], [int(mm[3 + k]) for k in range(3)]
    shift = lo if min(lo) < 0 else [0, 0, 0]                       # BSO:36-39
    dx, dy, dz = (hi[k] - shift[k] + 1 for k in range(3))          # BSO:40-41
    occ = torch.empty((dz, dy, dx), dtype=torch.int32, device=dev)
    sh = (ctypes.c_int32 * 3)(*shift)
    _call(dev, "vp_scatter_occupancy", coords.data_ptr(), N, sh, dz, dy, dx, occ.data_ptr(), scratch.data_ptr())
    return occ, lo


_agg_cache = {}


def aggregate_view_f16(view_sum, view_count, run16, views, first_view, view_index, nonfinite, flag_index=0, stream=None):
    """vp_aggregate_view_f16 (aggregate_voxel_features_onthefly.py:307-313 over the rows hit in this view; leaves
    view_sum / view_count zeroed).  ``nonfinite`` int32 tensor, element ``flag_index`` receives the view's NaN/Inf flag.
    Asynchronous on ``stream`` (a raw hipStream_t value; default: torch's current stream).  The tensors' checks and
    pointers are cached per argument set (the aggregator calls this once per view with the same tensors)."""
    import torch
    # the cache key holds the SHAPES as well as the addresses: the caching allocator hands freed addresses out again, and a
    # second aggregator with fewer rows or channels can receive the very same six pointers
    key = (view_sum.data_ptr(), view_count.data_ptr(), run16.data_ptr(), views.data_ptr(), first_view.data_ptr(), nonfinite.data_ptr(),
           tuple(view_sum.shape), tuple(run16.shape), view_count.numel(), views.numel(), first_view.numel())
    c = _agg_cache.get("k")
    if c is None or c[0] != key:
        n_rows, C = (int(v) for v in view_sum.shape)
        assert view_sum.dtype == torch.float32 and view_sum.is_contiguous() and view_count.dtype == torch.int32
        assert run16.dtype == torch.float16 and run16.is_contiguous() and tuple(run16.shape) == (n_rows, C)
        assert views.dtype == torch.int32 and first_view.dtype == torch.int32 and nonfinite.dtype == torch.int32
        assert view_count.numel() == n_rows and views.numel() == n_rows and first_view.numel() == n_rows
        assert view_count.is_contiguous() and views.is_contiguous() and first_view.is_contiguous()
        c = _agg_cache["k"] = (key, n_rows, C, lib().vp_aggregate_view_f16, view_sum.device)
    _, n_rows, C, fn, dev = c
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    assert 0 <= flag_index < nonfinite.numel()
    if torch.cuda.current_device() != dev.index:
        torch.cuda.set_device(dev)
    check(fn(key[0], key[1], key[2], key[3], key[4], int(view_index), key[5] + 4 * int(flag_index), n_rows, C, stream))


class _ContiguousDeviceMemory:
    """Owner of one hipExtMallocWithFlags(hipDeviceMallocContiguous) allocation, exported to torch through the CUDA array
    interface (torch keeps this object alive for as long as a tensor views the memory; freeing happens here)."""

    _hip = None

    def __init__(self, nbytes, shape, typestr, flags=0x4):
        cls = _ContiguousDeviceMemory
        if cls._hip is None:
            cls._hip = ctypes.CDLL("libamdhip64.so")
            cls._hip.hipExtMallocWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
            cls._hip.hipExtMallocWithFlags.restype = ctypes.c_int
            cls._hip.hipFree.argtypes = [ctypes.c_void_p]
        p = ctypes.c_void_p()
        # 0x4 hipDeviceMallocContiguous (default); experiments also use 0x1 hipDeviceMallocFinegrained, 0x3 hipDeviceMallocUncached
        rc = cls._hip.hipExtMallocWithFlags(ctypes.byref(p), max(int(nbytes), 256), int(flags))
        if rc != 0 or not p.value:
            raise MemoryError(f"hipExtMallocWithFlags(flags {flags:#x}, {nbytes} bytes) failed: hip error {rc}")
        self.ptr = p.value
        self.__cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": typestr, "data": (self.ptr, False),
                                         "version": 2}

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                self._hip.hipFree(ctypes.c_void_p(self.ptr))        # hipFree waits for the device to be done with it
                self.ptr = None
        except Exception:
            pass


def resident_empty(shape, dtype, device, fallback=True, flags=0x4):
    """An uninitialised CUDA tensor for a long-lived, heavily gathered buffer (the resident feature maps, the output rows)
    in PHYSICALLY CONTIGUOUS device memory (hipExtMallocWithFlags, hipDeviceMallocContiguous).  An experiment on the
    placement spread of DESIGN.md section 4 (round 2's probe, in git history): inside one process a 17 GB pool re-allocated this way
    kept one speed level (2.700-2.705 ms per 16-view launch, against 2.72-3.09 ms over plain re-allocations), but a 35 GB
    pool showed no difference and the spread between processes stayed -- so nothing uses it by default (bench.py --alloc
    contiguous).  With ``fallback`` a failed contiguous allocation (no contiguous range that large) falls back to torch's
    allocator.  Returns (tensor, "contiguous" | "default")."""
    import torch
    dev = torch.device(device)
    typestr = {torch.float32: "<f4", torch.float16: "<f2", torch.int32: "<i4", torch.int64: "<i8", torch.uint8: "|u1"}[dtype]
    n = 1
    for v in shape:
        n *= int(v)
    try:
        with torch.cuda.device(dev):
            mem = _ContiguousDeviceMemory(n * torch.empty((), dtype=dtype).element_size(), shape, typestr, flags)
            return torch.as_tensor(mem, device=dev), "contiguous"
    except (MemoryError, OSError):
        if not fallback:
            raise
        return torch.empty(tuple(int(v) for v in shape), dtype=dtype, device=dev), "default"


def stream_read_gbs(buf, repeats=3):
    """Measured streaming-read rate (GB/s) of this GPU over the float32 CUDA tensor ``buf`` (non-temporal loads)."""
    import torch
    L = lib()
    sink = torch.zeros(4, dtype=torch.float32, device=buf.device)
    n = (buf.numel() * buf.element_size() // 16) * 4
    stream = torch.cuda.current_stream(buf.device).cuda_stream
    check(L.vp_stream_read(buf.data_ptr(), n, sink.data_ptr(), stream))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        check(L.vp_stream_read(buf.data_ptr(), n, sink.data_ptr(), stream))
    e1.record()
    e1.synchronize()
    return n * 4 * repeats / (e0.elapsed_time(e1) * 1e-3) / 1e9
