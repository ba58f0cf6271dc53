"""ctypes binding of librigidbody_bindings.so (include/rigidbody.h + rigidbody_batch.h).

Host-side mirror of the reference's interface for the hot path:

* `Multibody.new()` / `.from_urdf(path)` / `.from_urdf_string(xml)` <- `multibody_new`,
  `Multibody::from_urdf` (rigidbody_bindings/src/lib.rs:8-12, multibody.rs:65-77)
* `.rnea(q, dq, ddq)`, `.crba(q)`, `.fwd_kin(q)`, `.jac(q)` <- the single-config C ABI
  (lib.rs:15-70), same argument meaning and result layout; computed on the calling thread
  with the GPU lane bodies compiled for the host (`.single_config_path()`), or on the GPU
* `.rnea_batch`, `.fd_batch`, `.crba_batch`, `.fwd_kin_batch`, `.jac_batch` <- batched
  device-pointer entry points on torch CUDA tensors laid out [n, B] (SoA)

Errors: the reference panics (aborting across FFI) on a bad URDF, a wrong DOF or a
NULL handle; here every failure raises RigidBodyError with the library's message.

torch is imported before the library is loaded on purpose: torch ships its own
libamdhip64.so.7 and the dynamic loader then binds this library to that same
runtime (same SONAME), so torch tensors, streams and these kernels share one HIP
runtime.  There is no CPU fallback: if the library is missing this import fails.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch  # noqa: F401  -- must precede the CDLL load (shared HIP runtime)

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RIGIDBODY_AMD_LIB", os.path.join(_PKG, "librigidbody_bindings.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
        "or make -C rigidbody-rs_amd)")

_lib = ctypes.CDLL(LIB_PATH)

_int, _uint, _i64, _u64, _size = ctypes.c_int, ctypes.c_uint, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
_dbl, _str, _vp = ctypes.c_double, ctypes.c_char_p, ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)

# exported symbols declared in include/*.h (tests check the list against the headers)
REFERENCE_SYMBOLS = ["multibody_new", "multibody_fwd_kin", "multibody_jac", "multibody_rnea",
                     "multibody_crba", "multibody_free"]
KINDS = {"rnea": 0, "fd": 1, "crba": 2, "rollout": 3, "fwd_kin": 4, "jac": 5, "rnea_fd": 6, "rnea_deriv": 7,
         "fd_deriv": 8}
GENERAL_AXES, URDF_TREE, FLOATING_BASE = 1, 2, 4  # rigidbody_batch.h RB_MODEL_*
TILE = 256  # configurations per tile of the tiled layout (rigidbody_batch.h)

# name -> (restype, argtypes); the handle and device / host arrays are void pointers
_SIGNATURES = {
    # the reference ABI (rigidbody.h)
    "multibody_new": (_vp, []),
    "multibody_free": (None, [_vp]),
    "multibody_fwd_kin": (_dp, [_vp, _dp]),
    "multibody_jac": (_dp, [_vp, _dp]),
    "multibody_crba": (_dp, [_vp, _dp]),
    "multibody_rnea": (_dp, [_vp, _dp, _dp, _dp]),
    # model construction and properties
    "multibody_new_from_urdf": (_vp, [_str]),
    "multibody_new_from_urdf_string": (_vp, [_str, _size]),
    "multibody_new_from_urdf_ex": (_vp, [_str, _uint]),
    "multibody_new_from_urdf_string_ex": (_vp, [_str, _size, _uint]),
    "multibody_new_from_blob": (_vp, [_dp, _i64]),
    "multibody_export_blob": (_int, [_vp, _dp, _i64]),
    "multibody_blob_size": (_i64, [_vp]),
    "multibody_flags": (_uint, [_vp]),
    "multibody_dof": (_int, [_vp]),
    "multibody_total_mass": (_dbl, [_vp]),
    "multibody_limits": (_int, [_vp, _dp, _dp, _dp, _dp]),
    "multibody_topology": (_int, [_vp, _ip, _ip]),
    "multibody_supported_dofs": (_int, [_ip, _int]),
    "multibody_upload": (_int, [_vp]),
    # kernel inspection: (handle, kind, f64[, batch, tiled], ...)
    "multibody_rnea_kernel_path": (_int, [_vp, _int]),
    "multibody_single_config_path": (_int, [_vp]),
    "multibody_kernel_path": (_int, [_vp, _int, _int]),
    "multibody_kernel_path_ex": (_int, [_vp, _int, _int, _i64, _int]),
    "multibody_kernel_form_ex": (_int, [_vp, _int, _int, _i64, _int]),
    "multibody_jit_source": (_int, [_vp, _int, _int, _str, _i64]),
    "multibody_jit_source_ex": (_int, [_vp, _int, _int, _i64, _int, _str, _i64]),
    "multibody_jit_compile": (_i64, [_vp, _int, _int, _str]),
    "multibody_jit_compile_ex": (_i64, [_vp, _int, _int, _i64, _int, _str]),
    # process-wide
    "multibody_result_free": (None, [_dp]),
    "rb_last_error": (_str, []),
    "rb_version": (_str, []),
    "rb_set_tuning": (_int, [_str, _int]),
    # one configuration, fp64, on the calling thread
    "multibody_rnea_deriv": (_int, [_vp, _dp, _dp, _dp, _dp, _dp]),
    "multibody_fd_deriv": (_int, [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "multibody_rollout_vjp": (_int, [_vp, _dp, _dp, _dp, _dbl, _int] + [_dp] * 5),
    # inspection of the rollout gradient's kernel: (handle, f64, batch, ...)
    "multibody_rollout_vjp_jit_source": (_int, [_vp, _int, _i64, _str, _i64]),
    "multibody_rollout_vjp_jit_compile": (_i64, [_vp, _int, _i64, _str]),
    # external link wrenches: one configuration (handle, q, qd, qdd | tau, fext, out); inspection
    # (handle, fd, f64, batch, ...)
    "multibody_rnea_ext": (_int, [_vp] + [_dp] * 5),
    "multibody_fd_ext": (_int, [_vp] + [_dp] * 5),
    "multibody_ext_jit_source": (_int, [_vp, _int, _int, _i64, _str, _i64]),
    "multibody_ext_jit_compile": (_i64, [_vp, _int, _int, _i64, _str]),
    # reverse-mode gradient of the inverse dynamics: one configuration (handle, q, qd, qdd, fext, w, g_q,
    # g_qd, g_qdd, g_fext); inspection (handle, ext, f64, batch, ...)
    "multibody_rnea_vjp": (_int, [_vp] + [_dp] * 9),
    "multibody_rnea_vjp_jit_source": (_int, [_vp, _int, _int, _i64, _str, _i64]),
    "multibody_rnea_vjp_jit_compile": (_i64, [_vp, _int, _int, _i64, _str]),
    # reverse-mode gradient of the forward dynamics: one configuration (handle, q, qd, tau, fext, w, qdd,
    # g_q, g_qd, g_tau, g_fext); inspection (handle, ext, f64, batch, ...)
    "multibody_fd_vjp": (_int, [_vp] + [_dp] * 10),
    "multibody_fd_vjp_jit_source": (_int, [_vp, _int, _int, _i64, _str, _i64]),
    "multibody_fd_vjp_jit_compile": (_i64, [_vp, _int, _int, _i64, _str]),
    # kinematics of every link: one configuration (handle, q, pos, rot) / (handle, q, qd, vel);
    # inspection (handle, vel, f64, batch, ...)
    "multibody_link_pose": (_int, [_vp] + [_dp] * 3),
    "multibody_link_vel": (_int, [_vp] + [_dp] * 3),
    "multibody_link_kin_jit_source": (_int, [_vp, _int, _int, _i64, _str, _i64]),
    "multibody_link_kin_jit_compile": (_i64, [_vp, _int, _int, _i64, _str]),
    # centre of mass, centroidal momentum and energy, momentum matrix: one configuration (handle, q, com) /
    # (handle, q, qd, com, hg, energy) / (handle, q, ag); inspection (handle, which, f64, batch, ...)
    "multibody_com": (_int, [_vp] + [_dp] * 2),
    "multibody_centroidal": (_int, [_vp] + [_dp] * 5),
    "multibody_cmm": (_int, [_vp] + [_dp] * 2),
    "multibody_centroidal_jit_source": (_int, [_vp, _int, _int, _i64, _str, _i64]),
    "multibody_centroidal_jit_compile": (_i64, [_vp, _int, _int, _i64, _str]),
    # compliant ground contact: the handle that carries a set, its getter; one configuration
    # (handle, q, qd, fext, cforce) / (handle, q, qd, tau_seq, dt, K, traj); inspection (handle,
    # rollout, f64, batch, ...)
    "multibody_with_contacts": (_vp, [_vp, _vp]),
    "multibody_contact_model": (_int, [_vp, _vp]),
    "multibody_contact_wrench": (_int, [_vp] + [_dp] * 4),
    "multibody_rollout_contact": (_int, [_vp, _dp, _dp, _dp, _dbl, _int, _dp]),
    "multibody_contact_jit_source": (_int, [_vp, _int, _int, _i64, _str, _i64]),
    "multibody_contact_jit_compile": (_i64, [_vp, _int, _int, _i64, _str]),
    "multibody_rollout_contact_vjp": (_int, [_vp, _dp, _dp, _dp, _dbl, _int] + [_dp] * 5),
    "multibody_contact_vjp_jit_source": (_int, [_vp, _int, _i64, _str, _i64]),
    "multibody_contact_vjp_jit_compile": (_i64, [_vp, _int, _i64, _str]),
}
# batched entry points: (handle, arrays..., batch[, ld][, stream]) by their number of arrays
_ARRAYS = {"rnea": 4, "fd": 4, "rnea_fd": 6, "crba": 2, "fwd_kin": 2, "jac": 2, "rnea_deriv": 5, "fd_deriv": 7,
           "rnea_ext": 5, "fd_ext": 5, "link_pose": 3, "link_vel": 3, "contact_wrench": 4, "com": 2, "centroidal": 5,
           "cmm": 2, "rnea_vjp": 9, "rnea_vjp_plain": 7, "fd_vjp": 10, "fd_vjp_plain": 8}
for _t in ("f32", "f64"):
    for _k, _n in _ARRAYS.items():
        _SIGNATURES[f"multibody_{_k}_batch_{_t}"] = (_int, [_vp] * (1 + _n) + [_i64, _i64, _vp])
        if not _k.endswith(("_deriv", "_ext")) and not _k.startswith(("link_", "contact_", "com", "centroidal", "cmm",
                                                                      "rnea_vjp", "fd_vjp")):
            _SIGNATURES[f"multibody_{_k}_batch_tiled_{_t}"] = (_int, [_vp] * (1 + _n) + [_i64, _vp])
        if _k not in ("crba", "fwd_kin", "jac"):
            _SIGNATURES[f"multibody_{_k}_batch_host_{_t}"] = (_int, [_vp] * (1 + _n) + [_i64])
    _SIGNATURES[f"multibody_rollout_batch_{_t}"] = (_int, [_vp, _vp, _vp, _vp, _dbl, _int, _vp, _i64, _i64, _vp])
    _SIGNATURES[f"multibody_rollout_contact_batch_{_t}"] = _SIGNATURES[f"multibody_rollout_batch_{_t}"]
    _SIGNATURES[f"multibody_rollout_contact_batch_host_{_t}"] = (_int, [_vp, _vp, _vp, _vp, _dbl, _int, _vp, _i64])
    # (handle, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau[, work], batch[, ld, stream])
    _SIGNATURES[f"multibody_rollout_vjp_batch_{_t}"] = (_int, [_vp] * 4 + [_dbl, _int] + [_vp] * 6 + [_i64, _i64, _vp])
    _SIGNATURES[f"multibody_rollout_vjp_batch_host_{_t}"] = (_int, [_vp] * 4 + [_dbl, _int] + [_vp] * 5 + [_i64])
    for _k in ("batch", "batch_host"):
        _SIGNATURES[f"multibody_rollout_contact_vjp_{_k}_{_t}"] = _SIGNATURES[f"multibody_rollout_vjp_{_k}_{_t}"]
    _SIGNATURES[f"rb_fill_uniform_{_t}"] = (_int, [_vp, _int, _i64, _i64, _dp, _dp, _u64, _vp])
    _SIGNATURES[f"rb_to_tiled_{_t}"] = (_int, [_vp, _i64, _vp, _int, _i64, _vp])
    _SIGNATURES[f"rb_from_tiled_{_t}"] = (_int, [_vp, _vp, _i64, _int, _i64, _vp])
for _name, (_res, _args) in _SIGNATURES.items():
    _f = getattr(_lib, _name)
    _f.restype, _f.argtypes = _res, _args


class RigidBodyError(RuntimeError):
    pass


CONTACT_MAX_POINTS = 16


class _ContactModel(ctypes.Structure):
    """rb_contact_model (rigidbody_batch.h)."""
    _fields_ = [("n_points", _int), ("link", _int * CONTACT_MAX_POINTS),
                ("point", (_dbl * 3) * CONTACT_MAX_POINTS), ("normal", _dbl * 3), ("offset", _dbl),
                ("stiffness", _dbl), ("damping", _dbl), ("friction", _dbl), ("slip_velocity", _dbl)]


def last_error() -> str:
    return (_lib.rb_last_error() or b"").decode()


def version() -> str:
    return _lib.rb_version().decode()


def lib():
    return _lib


def supported_dofs():
    buf = (ctypes.c_int * 64)()
    n = _lib.multibody_supported_dofs(buf, 64)
    return [buf[i] for i in range(n)]


def set_tuning(key: str, value: int):
    """rb_set_tuning: process-wide knobs -- production "jit", "pack", "rnea_stream",
    "single_gpu"; the A/B selectors only with RB_EXPERIMENTAL=1 (csrc/tuning.hpp)."""
    _check(_lib.rb_set_tuning(key.encode(), int(value)), f"set_tuning({key})")


def _check(rc, what):
    if rc != 0:
        raise RigidBodyError(f"{what} failed (status {rc}): {last_error()}")


def _dvec(x, n):
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.shape != (n,):
        raise ValueError(f"expected {n} values, got shape {a.shape}")
    return a


def _take(ptr, count):
    if not ptr:
        raise RigidBodyError(last_error())
    out = np.ctypeslib.as_array(ptr, shape=(count,)).copy()
    _lib.multibody_result_free(ptr)
    return out


_TORCH_SUFFIX = {torch.float32: "f32", torch.float64: "f64"}


def _stream_ptr(stream, device=None):
    """The HIP stream a call is enqueued on: `stream`, else the current stream of `device`."""
    if stream is None:
        stream = torch.cuda.current_stream(device)
    elif device is not None and stream.device != device:
        raise ValueError(f"stream is on {stream.device}, the arrays on {device}")
    return ctypes.c_void_p(stream.cuda_stream)


def _one_device(ts):
    """All arrays of one call must live on one device: the library uploads the model and
    launches on the CURRENT device (hipGetDevice), so the caller makes it theirs
    (`with torch.cuda.device(dev)` around the call)."""
    devs = {t.device for t in ts}
    if len(devs) != 1:
        raise ValueError(f"all arrays of one call must be on one device, got {sorted(map(str, devs))}")
    return devs.pop()


def _host_soa(arrs, n, dtype):
    """[n, B] host arrays of one batched host call: same shape, n rows, converted to `dtype`
    (float64, the reference's Real, or float32 for the *_host_f32 entry points)."""
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise TypeError(f"dtype must be float64 or float32, got {dt}")
    out = [np.ascontiguousarray(x, dtype=dt) for x in arrs]
    for a in out:
        if a.ndim != 2 or a.shape[0] != n or a.shape != out[0].shape:
            raise ValueError(f"host batch arrays must all be [{n}, B], got {[x.shape for x in out]}")
    return out


def _soa(t, n, name, dtype=None, B=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) torch tensor of shape [n, B]")
    if t.dim() != 2 or t.shape[0] != n:
        raise ValueError(f"{name} must have shape [{n}, B], got {tuple(t.shape)}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} has dtype {t.dtype}, expected {dtype}")
    if B is not None and t.shape[1] != B:
        raise ValueError(f"{name} has batch {t.shape[1]}, expected {B}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} must be contiguous along the batch axis")
    return t


def _ld(t):
    """Leading dimension (row stride in elements) of an [n, B] tensor."""
    if t.shape[1] == 0:
        return 1
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if ld < t.shape[1]:
        raise ValueError("rows of an [n, B] array must not overlap (row stride < B)")
    return ld


def _same_ld(ts):
    lds = {_ld(t) for t in ts}
    if len(lds) != 1:
        raise ValueError("all [n, B] arrays of one call must share the leading dimension")
    return lds.pop()


class Multibody:
    """Handle to a loaded serial chain (reference: `Multibody`, multibody.rs:32)."""

    def __init__(self, handle):
        if not handle:
            raise RigidBodyError(last_error())
        self._h = ctypes.c_void_p(handle)
        self.n = _lib.multibody_dof(self._h)

    # ------------------------------------------------------------------ construction
    @classmethod
    def new(cls):
        """multibody_new(): $RIGIDBODY_URDF, else the embedded FR3 model."""
        return cls(_lib.multibody_new())

    @classmethod
    def from_urdf(cls, path, flags: int = 0):
        """flags: GENERAL_AXES | URDF_TREE | FLOATING_BASE (rigidbody_batch.h RB_MODEL_*); 0 = the
        reference's reading."""
        if flags:
            return cls(_lib.multibody_new_from_urdf_ex(os.fsencode(path), flags))
        return cls(_lib.multibody_new_from_urdf(os.fsencode(path)))

    @classmethod
    def from_urdf_string(cls, xml: str, flags: int = 0):
        b = xml.encode()
        if flags:
            return cls(_lib.multibody_new_from_urdf_string_ex(b, len(b), flags))
        return cls(_lib.multibody_new_from_urdf_string(b, len(b)))

    @property
    def flags(self) -> int:
        return int(_lib.multibody_flags(self._h))

    @classmethod
    def from_blob(cls, blob):
        a = np.ascontiguousarray(blob, dtype=np.float64)
        return cls(_lib.multibody_new_from_blob(a.ctypes.data_as(_dp), a.size))

    def blob(self) -> np.ndarray:
        size = _lib.multibody_blob_size(self._h)
        out = np.zeros(size, dtype=np.float64)
        _check(_lib.multibody_export_blob(self._h, out.ctypes.data_as(_dp), size), "export_blob")
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.multibody_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def total_mass(self) -> float:
        return _lib.multibody_total_mass(self._h)

    def limits(self):
        arrs = [np.zeros(self.n) for _ in range(4)]
        _check(_lib.multibody_limits(self._h, *[a.ctypes.data_as(_dp) for a in arrs]), "limits")
        return tuple(arrs)  # lower, upper, velocity, effort

    def topology(self):
        """(parent [n] (-1 = base), joint_type [n] (0 revolute, 1 prismatic))."""
        par, typ = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        _check(_lib.multibody_topology(self._h, par.ctypes.data_as(_ip), typ.ctypes.data_as(_ip)), "topology")
        return par, typ

    def upload(self):
        _check(_lib.multibody_upload(self._h), "upload")

    def kernel_path(self, kind="rnea", f64=False, batch=1 << 20, tiled=False) -> str:
        """'jit' if the model-specialised hipRTC kernel of `kind` runs on this device for a
        launch of `batch` configurations (tiled: the *_tiled entry points)."""
        r = _lib.multibody_kernel_path_ex(self._h, KINDS[kind], int(bool(f64)), int(batch), int(bool(tiled)))
        if r < 0:
            raise RigidBodyError(last_error())
        return "jit" if r == 1 else "generic"

    def kernel_form(self, kind="rnea", f64=False, batch=1 << 20, tiled=False) -> int:
        """Configurations-per-lane form of the kernel such a launch takes (rigidbody_batch.h
        multibody_kernel_form_ex): 0 generic, 1 one per lane, 2 packed pair, 3 sequential pair,
        4 / 5 the packed / one-per-lane wave split."""
        r = _lib.multibody_kernel_form_ex(self._h, KINDS[kind], int(bool(f64)), int(batch), int(bool(tiled)))
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def single_config_path(self) -> str:
        """'host' when the single-configuration queries (rnea, crba, fwd_kin, jac) run on the
        calling thread (host_eval.cpp), 'gpu' when each is a GPU launch."""
        r = _lib.multibody_single_config_path(self._h)
        if r < 0:
            raise RigidBodyError(last_error())
        return "host" if r == 0 else "gpu"

    def rnea_kernel_path(self, f64=False) -> str:
        return self.kernel_path("rnea", f64)

    def jit_source(self, f64=False, kind="rnea", batch=1 << 20, tiled=False) -> str:
        """hipRTC source of the kernel a launch of `batch` configurations takes (tiled: the
        *_tiled entry points) -- multibody_jit_source_ex."""
        k, f, b, t = KINDS[kind], int(bool(f64)), int(batch), int(bool(tiled))
        n = _lib.multibody_jit_source_ex(self._h, k, f, b, t, None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        _lib.multibody_jit_source_ex(self._h, k, f, b, t, buf, n + 1)
        return buf.value.decode()

    def jit_compile(self, f64=False, arch="gfx950", kind="rnea", batch=1 << 20, tiled=False) -> int:
        r = _lib.multibody_jit_compile_ex(self._h, KINDS[kind], int(bool(f64)), int(batch), int(bool(tiled)),
                                          arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    # ------------------------------------------------- single configuration (ABI)
    def rnea(self, q, dq, ddq) -> np.ndarray:
        q, dq, ddq = (_dvec(x, self.n) for x in (q, dq, ddq))
        return _take(_lib.multibody_rnea(self._h, q.ctypes.data_as(_dp), dq.ctypes.data_as(_dp),
                                         ddq.ctypes.data_as(_dp)), self.n)

    def crba_raw(self, q) -> np.ndarray:
        """n*n column-major buffer exactly as multibody_crba returns it."""
        q = _dvec(q, self.n)
        return _take(_lib.multibody_crba(self._h, q.ctypes.data_as(_dp)), self.n * self.n)

    def crba(self, q) -> np.ndarray:
        return self.crba_raw(q).reshape(self.n, self.n).T.copy()

    def fwd_kin(self, q) -> np.ndarray:
        q = _dvec(q, self.n)
        return _take(_lib.multibody_fwd_kin(self._h, q.ctypes.data_as(_dp)), 3)

    def jac_raw(self, q) -> np.ndarray:
        q = _dvec(q, self.n)
        return _take(_lib.multibody_jac(self._h, q.ctypes.data_as(_dp)), 6 * self.n)

    def jac(self, q) -> np.ndarray:
        return self.jac_raw(q).reshape(self.n, 6).T.copy()

    def rnea_deriv(self, q, qd, qdd):
        """multibody_rnea_deriv: (dtau_dq, dtau_dqd), each (n, n) with [i, k] = d tau_i / d q_k
        (d qd_k), of tau = rnea(q, qd, qdd); one configuration, on the calling thread."""
        q, qd, qdd = (_dvec(x, self.n) for x in (q, qd, qdd))
        outs = [np.empty(self.n * self.n) for _ in range(2)]
        _check(_lib.multibody_rnea_deriv(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, qdd, *outs)]), "rnea_deriv")
        return tuple(o.reshape(self.n, self.n).T.copy() for o in outs)

    def fd_deriv(self, q, qd, tau):
        """multibody_fd_deriv: (qdd, dqdd_dq, dqdd_dqd, dqdd_dtau) of qdd = fd(q, qd, tau); the
        matrices (n, n) with [i, k] = d qdd_i / d q_k (d qd_k, d tau_k); one configuration, host."""
        q, qd, tau = (_dvec(x, self.n) for x in (q, qd, tau))
        qdd = np.empty(self.n)
        outs = [np.empty(self.n * self.n) for _ in range(3)]
        _check(_lib.multibody_fd_deriv(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, tau, qdd, *outs)]), "fd_deriv")
        return (qdd, *(o.reshape(self.n, self.n).T.copy() for o in outs))

    def rollout_vjp(self, q, qd, tau_seq, dt, gq, gqd, _op="rollout_vjp"):
        """multibody_rollout_vjp: (g_q0 [n], g_qd0 [n], g_tau [K, n]), the gradient of
        sum_k gq[k] . q_{k+1} + gqd[k] . qd_{k+1} over the K-step rollout from (q, qd) under tau_seq
        [K, n]; gq, gqd [K, n].  One configuration, on the calling thread."""
        q, qd = (_dvec(x, self.n) for x in (q, qd))
        tau_seq, gq, gqd = (np.ascontiguousarray(x, dtype=np.float64) for x in (tau_seq, gq, gqd))
        K = tau_seq.shape[0] if tau_seq.ndim == 2 else -1
        for a in (tau_seq, gq, gqd):
            if a.shape != (K, self.n):
                raise ValueError(f"tau_seq, gq and gqd must all be [K, {self.n}], got {a.shape}")
        outs = [np.empty(self.n), np.empty(self.n), np.empty((K, self.n))]
        _check(getattr(_lib, f"multibody_{_op}")(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, tau_seq)], float(dt), K,
                                                 *[a.ctypes.data_as(_dp) for a in (gq, gqd, *outs)]), _op)
        return tuple(outs)

    def rollout_contact_vjp(self, q, qd, tau_seq, dt, gq, gqd):
        """multibody_rollout_contact_vjp: rollout_vjp through the contact rollout of a handle that carries
        a contact set (rollout_contact's trajectory on the mass-matrix forward dynamics)."""
        return self.rollout_vjp(q, qd, tau_seq, dt, gq, gqd, _op="rollout_contact_vjp")

    def rollout_vjp_jit_source(self, f64=False, batch=1 << 20, _op="rollout_vjp") -> str:
        """hipRTC source of the rollout gradient's kernel (multibody_rollout_vjp_jit_source); the
        empty string for a model outside its scope."""
        fn = getattr(_lib, f"multibody_{_op}_jit_source")
        n = fn(self._h, int(bool(f64)), int(batch), None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        fn(self._h, int(bool(f64)), int(batch), buf, n + 1)
        return buf.value.decode()

    def rollout_vjp_jit_compile(self, f64=False, arch="gfx950", batch=1 << 20, _op="rollout_vjp") -> int:
        r = getattr(_lib, f"multibody_{_op}_jit_compile")(self._h, int(bool(f64)), int(batch), arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def contact_vjp_jit_source(self, f64=False, batch=1 << 20) -> str:
        """hipRTC source of the contact rollout gradient's kernel (multibody_contact_vjp_jit_source); the
        empty string for a model outside its scope or without a contact set."""
        return self.rollout_vjp_jit_source(f64, batch, _op="contact_vjp")

    def contact_vjp_jit_compile(self, f64=False, arch="gfx950", batch=1 << 20) -> int:
        return self.rollout_vjp_jit_compile(f64, arch, batch, _op="contact_vjp")

    # ---- external link wrenches: fext holds link j's force then its moment, in its URDF link frame
    def rnea_ext(self, q, qd, qdd, fext) -> np.ndarray:
        """multibody_rnea_ext: tau = rnea(q, qd, qdd) - sum_j J_j^T fext_j; fext [6 n] (or [n, 6]).  One
        configuration, on the calling thread."""
        return self._ext_single(_lib.multibody_rnea_ext, "rnea_ext", q, qd, qdd, fext)

    def fd_ext(self, q, qd, tau, fext) -> np.ndarray:
        """multibody_fd_ext: qdd = fd(q, qd, tau + sum_j J_j^T fext_j); as rnea_ext."""
        return self._ext_single(_lib.multibody_fd_ext, "fd_ext", q, qd, tau, fext)

    def _ext_single(self, fn, what, q, qd, third, fext):
        q, qd, third = (_dvec(x, self.n) for x in (q, qd, third))
        fext = _dvec(np.asarray(fext, dtype=np.float64).reshape(-1), 6 * self.n)
        out = np.empty(self.n)
        _check(fn(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, third, fext, out)]), what)
        return out

    def ext_jit_source(self, fd=False, f64=False, batch=1 << 20) -> str:
        """hipRTC source of the rnea_ext (fd=False) / fd_ext (fd=True) kernel (multibody_ext_jit_source)."""
        a = (self._h, int(bool(fd)), int(bool(f64)), int(batch))
        n = _lib.multibody_ext_jit_source(*a, None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        _lib.multibody_ext_jit_source(*a, buf, n + 1)
        return buf.value.decode()

    def ext_jit_compile(self, fd=False, f64=False, arch="gfx950", batch=1 << 20) -> int:
        r = _lib.multibody_ext_jit_compile(self._h, int(bool(fd)), int(bool(f64)), int(batch), arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def _ext_call(self, kind, q, qd, third, third_name, fext, out, out_name, stream):
        q = _soa(q, self.n, "q")
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"q has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        qd = _soa(qd, self.n, "qd", q.dtype, B)
        third = _soa(third, self.n, third_name, q.dtype, B)
        fext = _soa(fext, 6 * self.n, "fext", q.dtype, B)
        if out is None:
            out = torch.empty((self.n, _ld(q)), dtype=q.dtype, device=q.device)[:, :B]
        else:
            _soa(out, self.n, out_name, q.dtype, B)
        live = (q, qd, third, fext, out)
        ld = _same_ld(live)
        dev = _one_device(live)
        fn = getattr(_lib, f"multibody_{kind}_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, *[t.data_ptr() for t in live], B, ld, _stream_ptr(stream, dev)), f"{kind}_batch")
        return out

    def rnea_ext_batch(self, q, qd, qdd, fext, out=None, stream=None):
        """multibody_rnea_ext_batch_*: q, qd, qdd [n, B], fext [6 n, B] (row 6 j + c: component c of
        the wrench on link j, force then moment, in link j's URDF frame) -> tau [n, B]."""
        return self._ext_call("rnea_ext", q, qd, qdd, "qdd", fext, out, "tau", stream)

    def fd_ext_batch(self, q, qd, tau, fext, out=None, stream=None):
        """multibody_fd_ext_batch_*: as rnea_ext_batch -> qdd [n, B]."""
        return self._ext_call("fd_ext", q, qd, tau, "tau", fext, out, "qdd", stream)

    def _ext_host(self, kind, q, qd, third, fext, dtype):
        arrs = _host_soa((q, qd, third), self.n, dtype)
        B = arrs[0].shape[1]
        fext = np.ascontiguousarray(fext, dtype=arrs[0].dtype)
        if fext.shape != (6 * self.n, B):
            raise ValueError(f"fext must be [{6 * self.n}, {B}], got {fext.shape}")
        out = np.empty((self.n, B), dtype=arrs[0].dtype)
        fn = getattr(_lib, f"multibody_{kind}_batch_host_{'f32' if out.dtype == np.float32 else 'f64'}")
        _check(fn(self._h, *[a.ctypes.data for a in (*arrs, fext, out)], B), f"{kind}_batch_host")
        return out

    def rnea_ext_batch_host(self, q, qd, qdd, fext, dtype=np.float64):
        """Blocking host form of rnea_ext_batch on numpy arrays."""
        return self._ext_host("rnea_ext", q, qd, qdd, fext, dtype)

    def fd_ext_batch_host(self, q, qd, tau, fext, dtype=np.float64):
        """Blocking host form of fd_ext_batch on numpy arrays."""
        return self._ext_host("fd_ext", q, qd, tau, fext, dtype)

    # ---- reverse-mode gradient of the inverse dynamics (rigidbody_batch.h has the definitions)
    def rnea_vjp(self, q, qd, qdd, w, fext=None):
        """multibody_rnea_vjp: (g_q, g_qd, g_qdd [n][, g_fext [n, 6]]), the gradient of w . rnea_ext(q, qd, qdd,
        fext) -- fext=None: of w . rnea(q, qd, qdd) -- of one configuration, on the calling thread."""
        q, qd, qdd, w = (_dvec(x, self.n) for x in (q, qd, qdd, w))
        outs = [np.empty(self.n) for _ in range(3)]
        gf = None
        if fext is not None:
            fext = _dvec(np.asarray(fext, dtype=np.float64).reshape(-1), 6 * self.n)
            gf = np.empty(6 * self.n)
        ptr = lambda a: None if a is None else a.ctypes.data_as(_dp)
        _check(_lib.multibody_rnea_vjp(self._h, *[ptr(a) for a in (q, qd, qdd, fext, w, *outs, gf)]), "rnea_vjp")
        return (*outs, gf.reshape(self.n, 6)) if gf is not None else tuple(outs)

    def rnea_vjp_jit_source(self, ext=False, f64=False, batch=1 << 20) -> str:
        """hipRTC source of the rnea_vjp kernel without (ext=False) / with wrench rows
        (multibody_rnea_vjp_jit_source)."""
        a = (self._h, int(bool(ext)), int(bool(f64)), int(batch))
        n = _lib.multibody_rnea_vjp_jit_source(*a, None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        _lib.multibody_rnea_vjp_jit_source(*a, buf, n + 1)
        return buf.value.decode()

    def rnea_vjp_jit_compile(self, ext=False, f64=False, arch="gfx950", batch=1 << 20) -> int:
        r = _lib.multibody_rnea_vjp_jit_compile(self._h, int(bool(ext)), int(bool(f64)), int(batch), arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def rnea_vjp_batch(self, q, qd, qdd, w, fext=None, stream=None):
        """multibody_rnea_vjp_batch_* (fext [6 n, B]) / multibody_rnea_vjp_plain_batch_* (fext=None): q, qd,
        qdd, w [n, B] -> (g_q, g_qd, g_qdd [n, B][, g_fext [6 n, B]]), the gradient of sum_i w_i tau_i per
        configuration; rows of g_fext as those of fext."""
        q = _soa(q, self.n, "q")
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"q has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        ins = [q] + [_soa(t, self.n, name, q.dtype, B) for t, name in ((qd, "qd"), (qdd, "qdd"))]
        if fext is not None:
            ins.append(_soa(fext, 6 * self.n, "fext", q.dtype, B))
        ins.append(_soa(w, self.n, "w", q.dtype, B))
        rows = [self.n] * 3 + ([6 * self.n] if fext is not None else [])
        outs = [torch.empty((r, _ld(q)), dtype=q.dtype, device=q.device)[:, :B] for r in rows]
        live = ins + outs
        ld = _same_ld(live)
        dev = _one_device(live)
        kind = "rnea_vjp" if fext is not None else "rnea_vjp_plain"
        fn = getattr(_lib, f"multibody_{kind}_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, *[t.data_ptr() for t in live], B, ld, _stream_ptr(stream, dev)), f"{kind}_batch")
        return tuple(outs)

    def rnea_vjp_batch_host(self, q, qd, qdd, w, fext=None, dtype=np.float64):
        """Blocking host form of rnea_vjp_batch on numpy arrays."""
        arrs = _host_soa((q, qd, qdd, w), self.n, dtype)
        B = arrs[0].shape[1]
        ins = list(arrs[:3])
        if fext is not None:
            fext = np.ascontiguousarray(fext, dtype=arrs[0].dtype)
            if fext.shape != (6 * self.n, B):
                raise ValueError(f"fext must be [{6 * self.n}, {B}], got {fext.shape}")
            ins.append(fext)
        ins.append(arrs[3])
        rows = [self.n] * 3 + ([6 * self.n] if fext is not None else [])
        outs = [np.empty((r, B), dtype=arrs[0].dtype) for r in rows]
        kind = "rnea_vjp" if fext is not None else "rnea_vjp_plain"
        fn = getattr(_lib, f"multibody_{kind}_batch_host_{'f32' if arrs[0].dtype == np.float32 else 'f64'}")
        _check(fn(self._h, *[a.ctypes.data for a in (*ins, *outs)], B), f"{kind}_batch_host")
        return tuple(outs)

    # ---- reverse-mode gradient of the forward dynamics (rigidbody_batch.h has the definitions)
    def fd_vjp(self, q, qd, tau, w, fext=None):
        """multibody_fd_vjp: (qdd, g_q, g_qd, g_tau [n][, g_fext [n, 6]]), qdd = fd_ext(q, qd, tau, fext) -- fext=None:
        without wrenches -- and the gradient of w . qdd, of one configuration, on the calling thread."""
        q, qd, tau, w = (_dvec(x, self.n) for x in (q, qd, tau, w))
        outs = [np.empty(self.n) for _ in range(4)]
        gf = None
        if fext is not None:
            fext = _dvec(np.asarray(fext, dtype=np.float64).reshape(-1), 6 * self.n)
            gf = np.empty(6 * self.n)
        ptr = lambda a: None if a is None else a.ctypes.data_as(_dp)
        _check(_lib.multibody_fd_vjp(self._h, *[ptr(a) for a in (q, qd, tau, fext, w, *outs, gf)]), "fd_vjp")
        return (*outs, gf.reshape(self.n, 6)) if gf is not None else tuple(outs)

    def fd_vjp_jit_source(self, ext=False, f64=False, batch=1 << 20) -> str:
        """hipRTC source of the fd_vjp kernel without (ext=False) / with wrench rows
        (multibody_fd_vjp_jit_source)."""
        a = (self._h, int(bool(ext)), int(bool(f64)), int(batch))
        n = _lib.multibody_fd_vjp_jit_source(*a, None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        _lib.multibody_fd_vjp_jit_source(*a, buf, n + 1)
        return buf.value.decode()

    def fd_vjp_jit_compile(self, ext=False, f64=False, arch="gfx950", batch=1 << 20) -> int:
        r = _lib.multibody_fd_vjp_jit_compile(self._h, int(bool(ext)), int(bool(f64)), int(batch), arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def fd_vjp_batch(self, q, qd, tau, w, fext=None, stream=None):
        """multibody_fd_vjp_batch_* (fext [6 n, B]) / multibody_fd_vjp_plain_batch_* (fext=None): q, qd, tau,
        w [n, B] -> (qdd, g_q, g_qd, g_tau [n, B][, g_fext [6 n, B]]): the forward dynamics and the gradient
        of sum_i w_i qdd_i per configuration, one launch; rows of g_fext as those of fext."""
        q = _soa(q, self.n, "q")
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"q has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        ins = [q] + [_soa(t, self.n, name, q.dtype, B) for t, name in ((qd, "qd"), (tau, "tau"))]
        if fext is not None:
            ins.append(_soa(fext, 6 * self.n, "fext", q.dtype, B))
        ins.append(_soa(w, self.n, "w", q.dtype, B))
        rows = [self.n] * 4 + ([6 * self.n] if fext is not None else [])
        outs = [torch.empty((r, _ld(q)), dtype=q.dtype, device=q.device)[:, :B] for r in rows]
        live = ins + outs
        ld = _same_ld(live)
        dev = _one_device(live)
        kind = "fd_vjp" if fext is not None else "fd_vjp_plain"
        fn = getattr(_lib, f"multibody_{kind}_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, *[t.data_ptr() for t in live], B, ld, _stream_ptr(stream, dev)), f"{kind}_batch")
        return tuple(outs)

    def fd_vjp_batch_host(self, q, qd, tau, w, fext=None, dtype=np.float64):
        """Blocking host form of fd_vjp_batch on numpy arrays."""
        arrs = _host_soa((q, qd, tau, w), self.n, dtype)
        B = arrs[0].shape[1]
        ins = list(arrs[:3])
        if fext is not None:
            fext = np.ascontiguousarray(fext, dtype=arrs[0].dtype)
            if fext.shape != (6 * self.n, B):
                raise ValueError(f"fext must be [{6 * self.n}, {B}], got {fext.shape}")
            ins.append(fext)
        ins.append(arrs[3])
        rows = [self.n] * 4 + ([6 * self.n] if fext is not None else [])
        outs = [np.empty((r, B), dtype=arrs[0].dtype) for r in rows]
        kind = "fd_vjp" if fext is not None else "fd_vjp_plain"
        fn = getattr(_lib, f"multibody_{kind}_batch_host_{'f32' if arrs[0].dtype == np.float32 else 'f64'}")
        _check(fn(self._h, *[a.ctypes.data for a in (*ins, *outs)], B), f"{kind}_batch_host")
        return tuple(outs)

    # ---- kinematics of every link, in its own URDF link frame (the frame fext is given in)
    def link_pose(self, q):
        """multibody_link_pose: (pos [n, 3], rot [n, 3, 3]) of one configuration, on the calling thread:
        link j's frame origin in the base frame and its rotation R_j, x_base = R_j x_link."""
        q = _dvec(q, self.n)
        pos, rot = np.empty(3 * self.n), np.empty(9 * self.n)
        _check(_lib.multibody_link_pose(self._h, *[a.ctypes.data_as(_dp) for a in (q, pos, rot)]), "link_pose")
        return pos.reshape(self.n, 3), rot.reshape(self.n, 3, 3).transpose(0, 2, 1)  # column-major per link

    def link_vel(self, q, qd):
        """multibody_link_vel: vel [n, 6] of one configuration: link j's linear, then angular velocity,
        in its own frame (vel_j = J_j(q) qd)."""
        q, qd = _dvec(q, self.n), _dvec(qd, self.n)
        vel = np.empty(6 * self.n)
        _check(_lib.multibody_link_vel(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, vel)]), "link_vel")
        return vel.reshape(self.n, 6)

    def link_kin_jit_source(self, vel=False, f64=False, batch=1 << 20) -> str:
        """hipRTC source of the link_pose (vel=False) / link_vel (vel=True) kernel
        (multibody_link_kin_jit_source)."""
        a = (self._h, int(bool(vel)), int(bool(f64)), int(batch))
        n = _lib.multibody_link_kin_jit_source(*a, None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        _lib.multibody_link_kin_jit_source(*a, buf, n + 1)
        return buf.value.decode()

    def link_kin_jit_compile(self, vel=False, f64=False, arch="gfx950", batch=1 << 20) -> int:
        r = _lib.multibody_link_kin_jit_compile(self._h, int(bool(vel)), int(bool(f64)), int(batch), arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def _link_kin_call(self, kind, ins, outs, stream):
        """ins: (tensor, name) pairs of [n, B] inputs; outs: (tensor or None, name, rows per link)."""
        q = _soa(ins[0][0], self.n, ins[0][1])
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"q has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        live = [q] + [_soa(t, self.n, name, q.dtype, B) for t, name in ins[1:]]
        res = []
        for t, name, rows in outs:
            if t is None:
                t = torch.empty((rows * self.n, _ld(q)), dtype=q.dtype, device=q.device)[:, :B]
            else:
                _soa(t, rows * self.n, name, q.dtype, B)
            res.append(t)
        live += res
        ld = _same_ld(live)
        dev = _one_device(live)
        fn = getattr(_lib, f"multibody_{kind}_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, *[t.data_ptr() for t in live], B, ld, _stream_ptr(stream, dev)), f"{kind}_batch")
        return res

    def link_pose_batch(self, q, pos=None, rot=None, stream=None):
        """multibody_link_pose_batch_*: q [n, B] -> (pos [3 n, B], rot [9 n, B]); row 3 j + c of pos is
        component c of link j's frame origin in the base frame, row 9 j + row + 3 col of rot the
        rotation R_j (x_base = R_j x_link)."""
        pos, rot = self._link_kin_call("link_pose", [(q, "q")], [(pos, "pos", 3), (rot, "rot", 9)], stream)
        return pos, rot

    def link_vel_batch(self, q, qd, out=None, stream=None):
        """multibody_link_vel_batch_*: q, qd [n, B] -> vel [6 n, B]; rows 6 j + 0..2 the linear, 6 j +
        3..5 the angular velocity of link j, in its own URDF link frame (the rows of fext)."""
        return self._link_kin_call("link_vel", [(q, "q"), (qd, "qd")], [(out, "vel", 6)], stream)[0]

    def _link_kin_host(self, kind, ins, rows, dtype):
        arrs = _host_soa(ins, self.n, dtype)
        B = arrs[0].shape[1]
        outs = [np.empty((r * self.n, B), dtype=arrs[0].dtype) for r in rows]
        fn = getattr(_lib, f"multibody_{kind}_batch_host_{'f32' if arrs[0].dtype == np.float32 else 'f64'}")
        _check(fn(self._h, *[a.ctypes.data for a in (*arrs, *outs)], B), f"{kind}_batch_host")
        return outs

    def link_pose_batch_host(self, q, dtype=np.float64):
        """Blocking host form of link_pose_batch on numpy arrays -> (pos, rot)."""
        return tuple(self._link_kin_host("link_pose", (q,), (3, 9), dtype))

    def link_vel_batch_host(self, q, qd, dtype=np.float64):
        """Blocking host form of link_vel_batch on numpy arrays."""
        return self._link_kin_host("link_vel", (q, qd), (6,), dtype)[0]

    # ---- centre of mass, centroidal momentum, energy (rigidbody_batch.h has the definitions)
    CENTROIDAL_KERNELS = {"com": 0, "centroidal": 1, "cmm": 2}

    def com(self, q) -> np.ndarray:
        """multibody_com: the centre of mass [3] in the base frame; one configuration, on the calling thread."""
        q, out = _dvec(q, self.n), np.empty(3)
        _check(_lib.multibody_com(self._h, q.ctypes.data_as(_dp), out.ctypes.data_as(_dp)), "com")
        return out

    def centroidal(self, q, qd):
        """multibody_centroidal: (com [3], hg [6], energy [2]) of one configuration: hg the linear momentum,
        then the angular momentum about com, base axes; energy (kinetic, potential = g M com_z)."""
        q, qd = _dvec(q, self.n), _dvec(qd, self.n)
        outs = [np.empty(3), np.empty(6), np.empty(2)]
        _check(_lib.multibody_centroidal(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, *outs)]), "centroidal")
        return tuple(outs)

    def cmm_raw(self, q) -> np.ndarray:
        """6 n column-major buffer exactly as multibody_cmm fills it."""
        q, out = _dvec(q, self.n), np.empty(6 * self.n)
        _check(_lib.multibody_cmm(self._h, q.ctypes.data_as(_dp), out.ctypes.data_as(_dp)), "cmm")
        return out

    def cmm(self, q) -> np.ndarray:
        """multibody_cmm: the centroidal momentum matrix A_G (6, n), hg = A_G qd."""
        return self.cmm_raw(q).reshape(self.n, 6).T.copy()

    def centroidal_jit_source(self, which="centroidal", f64=False, batch=1 << 20) -> str:
        """hipRTC source of the "com" / "centroidal" / "cmm" kernel (or 0 / 1 / 2;
        multibody_centroidal_jit_source)."""
        a = (self._h, int(self.CENTROIDAL_KERNELS.get(which, which)), int(bool(f64)), int(batch))
        n = _lib.multibody_centroidal_jit_source(*a, None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        _lib.multibody_centroidal_jit_source(*a, buf, n + 1)
        return buf.value.decode()

    def centroidal_jit_compile(self, which="centroidal", f64=False, arch="gfx950", batch=1 << 20) -> int:
        r = _lib.multibody_centroidal_jit_compile(self._h, int(self.CENTROIDAL_KERNELS.get(which, which)),
                                                  int(bool(f64)), int(batch), arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def com_batch(self, q, out=None, stream=None):
        """multibody_com_batch_*: q [n, B] -> com [3, B], base frame."""
        return self._soa_call("com", [(q, "q")], [(out, "com", 3)], stream)[0]

    def centroidal_batch(self, q, qd, com=None, hg=None, energy=None, stream=None):
        """multibody_centroidal_batch_*: q, qd [n, B] -> (com [3, B], hg [6, B], energy [2, B]): rows 0..2 of
        hg the linear momentum, 3..5 the angular momentum about com; energy row 0 T, row 1 U."""
        return tuple(self._soa_call("centroidal", [(q, "q"), (qd, "qd")],
                                    [(com, "com", 3), (hg, "hg", 6), (energy, "energy", 2)], stream))

    def cmm_batch(self, q, out=None, stream=None):
        """multibody_cmm_batch_*: q [n, B] -> ag [6 n, B], row r + 6 k: element (r, k) of A_G."""
        return self._soa_call("cmm", [(q, "q")], [(out, "ag", 6 * self.n)], stream)[0]

    def _centroidal_host(self, kind, ins, rows, dtype):
        arrs = _host_soa(ins, self.n, dtype)
        B = arrs[0].shape[1]
        outs = [np.empty((r, B), dtype=arrs[0].dtype) for r in rows]
        fn = getattr(_lib, f"multibody_{kind}_batch_host_{'f32' if arrs[0].dtype == np.float32 else 'f64'}")
        _check(fn(self._h, *[a.ctypes.data for a in (*arrs, *outs)], B), f"{kind}_batch_host")
        return outs

    def com_batch_host(self, q, dtype=np.float64):
        """Blocking host form of com_batch on numpy arrays."""
        return self._centroidal_host("com", (q,), (3,), dtype)[0]

    def centroidal_batch_host(self, q, qd, dtype=np.float64):
        """Blocking host form of centroidal_batch on numpy arrays -> (com, hg, energy)."""
        return tuple(self._centroidal_host("centroidal", (q, qd), (3, 6, 2), dtype))

    def cmm_batch_host(self, q, dtype=np.float64):
        """Blocking host form of cmm_batch on numpy arrays."""
        return self._centroidal_host("cmm", (q,), (6 * self.n,), dtype)[0]

    # ---- compliant ground contact (rigidbody_batch.h "compliant ground contact")
    def with_contacts(self, links, points, normal=(0.0, 0.0, 1.0), offset=0.0, stiffness=2000.0, damping=0.5,
                      friction=0.7, slip_velocity=0.01):
        """multibody_with_contacts: a NEW Multibody, this model plus a contact set -- points[p] (in the
        URDF link frame of moving link links[p]) against the plane normal . x = offset of the base
        frame, with the Hunt-Crossley / regularised-friction law's stiffness [N/m], damping [s/m],
        friction and slip_velocity [m/s].  This handle is not modified."""
        links = [int(l) for l in links]
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        if len(links) != len(pts):
            raise ValueError(f"{len(links)} links for {len(pts)} points")
        cm = _ContactModel()
        cm.n_points = len(links)
        for p in range(min(len(links), CONTACT_MAX_POINTS)):
            cm.link[p] = links[p]
            for k in range(3):
                cm.point[p][k] = pts[p, k]
        for k in range(3):
            cm.normal[k] = float(normal[k])
        cm.offset, cm.stiffness, cm.damping = float(offset), float(stiffness), float(damping)
        cm.friction, cm.slip_velocity = float(friction), float(slip_velocity)
        return Multibody(_lib.multibody_with_contacts(self._h, ctypes.byref(cm)))

    def contact_model(self):
        """multibody_contact_model: the contact set as a dict (None: the model carries none)."""
        cm = _ContactModel()
        P = _lib.multibody_contact_model(self._h, ctypes.byref(cm))
        if P < 0:
            raise RigidBodyError(last_error())
        if P == 0:
            return None
        return {"links": [cm.link[p] for p in range(P)],
                "points": np.array([[cm.point[p][k] for k in range(3)] for p in range(P)]),
                "normal": tuple(cm.normal[k] for k in range(3)), "offset": cm.offset, "stiffness": cm.stiffness,
                "damping": cm.damping, "friction": cm.friction, "slip_velocity": cm.slip_velocity}

    @property
    def n_contacts(self) -> int:
        P = _lib.multibody_contact_model(self._h, None)
        if P < 0:
            raise RigidBodyError(last_error())
        return P

    def contact_wrench(self, q, qd):
        """multibody_contact_wrench: (fext [n, 6], cforce [P, 3]) of one configuration, on the calling
        thread: the contact set's wrench on every link (its URDF link frame, [force; moment]) and the
        force at every point (base frame)."""
        q, qd = _dvec(q, self.n), _dvec(qd, self.n)
        fext, cforce = np.empty(6 * self.n), np.empty(3 * max(self.n_contacts, 1))
        _check(_lib.multibody_contact_wrench(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, fext, cforce)]),
               "contact_wrench")
        return fext.reshape(self.n, 6), cforce.reshape(-1, 3)[:self.n_contacts]

    def rollout_contact(self, q, qd, tau_seq, dt):
        """multibody_rollout_contact: K steps of one configuration on the calling thread; tau_seq
        [K, n].  Returns (traj [K, n], q [n], qd [n]) -- the inputs are not modified."""
        q, qd = _dvec(q, self.n).copy(), _dvec(qd, self.n).copy()
        tau = np.ascontiguousarray(tau_seq, dtype=np.float64)
        if tau.ndim != 2 or tau.shape[1] != self.n:
            raise ValueError(f"tau_seq must be [K, {self.n}]")
        traj = np.empty_like(tau)
        _check(_lib.multibody_rollout_contact(self._h, *[a.ctypes.data_as(_dp) for a in (q, qd, tau)], float(dt),
                                              tau.shape[0], traj.ctypes.data_as(_dp)), "rollout_contact")
        return traj, q, qd

    def contact_jit_source(self, rollout=False, f64=False, batch=1 << 20) -> str:
        """hipRTC source of the contact_wrench (rollout=False) / rollout_contact kernel
        (multibody_contact_jit_source)."""
        a = (self._h, int(bool(rollout)), int(bool(f64)), int(batch))
        n = _lib.multibody_contact_jit_source(*a, None, 0)
        if n < 0:
            raise RigidBodyError(last_error())
        buf = ctypes.create_string_buffer(n + 1)
        _lib.multibody_contact_jit_source(*a, buf, n + 1)
        return buf.value.decode()

    def contact_jit_compile(self, rollout=False, f64=False, arch="gfx950", batch=1 << 20) -> int:
        r = _lib.multibody_contact_jit_compile(self._h, int(bool(rollout)), int(bool(f64)), int(batch), arch.encode())
        if r < 0:
            raise RigidBodyError(last_error())
        return r

    def contact_wrench_batch(self, q, qd, fext=None, cforce=None, stream=None):
        """multibody_contact_wrench_batch_*: q, qd [n, B] -> (fext [6 n, B], cforce [3 P, B]); fext as
        rnea_ext_batch / fd_ext_batch take it, row 3 p + c of cforce component c of the force at
        point p in the base frame."""
        q = _soa(q, self.n, "q")
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"q has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        qd = _soa(qd, self.n, "qd", q.dtype, B)
        res = []
        for t, name, rows in ((fext, "fext", 6 * self.n), (cforce, "cforce", 3 * max(self.n_contacts, 1))):
            if t is None:
                t = torch.empty((rows, _ld(q)), dtype=q.dtype, device=q.device)[:, :B]
            else:
                _soa(t, rows, name, q.dtype, B)
            res.append(t)
        live = [q, qd] + res
        ld = _same_ld(live)
        dev = _one_device(live)
        fn = getattr(_lib, f"multibody_contact_wrench_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, *[t.data_ptr() for t in live], B, ld, _stream_ptr(stream, dev)), "contact_wrench_batch")
        return res[0], res[1]

    def rollout_contact_batch(self, q, qd, tau_seq, dt, traj=None, stream=None):
        """multibody_rollout_contact_batch_*: K fused steps of fd_ext under the contact set, in place on
        q and qd ([n, B] CUDA tensors); tau_seq [K, n, B].  Returns the trajectory [K, n, B] of q
        (allocated here unless given).  Rows may be longer than B: every array -- tau_seq and traj as
        [K n] rows -- shares one leading dimension."""
        q = _soa(q, self.n, "q")
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"q has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        qd = _soa(qd, self.n, "qd", q.dtype, B)
        ld = _same_ld((q, qd))

        def rows(t, name):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[1:] != (self.n, B) or t.dtype != q.dtype:
                raise ValueError(f"{name} must be [K, {self.n}, {B}] of the state's dtype")
            if t.numel() and B > 1 and (t.stride(2) != 1 or t.stride(1) != ld or t.stride(0) != self.n * ld):
                raise ValueError(f"{name} must be [K n] rows of the state's leading dimension ({ld})")
            return t

        tau_seq = rows(tau_seq, "tau_seq")
        K = tau_seq.shape[0]
        if traj is None:
            traj = torch.empty((K, self.n, max(ld, 1)), dtype=q.dtype, device=q.device)[:, :, :B]
        elif rows(traj, "traj").shape[0] != K:
            raise ValueError(f"traj must have {K} steps")
        dev = _one_device((q, qd, tau_seq, traj))
        fn = getattr(_lib, f"multibody_rollout_contact_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, q.data_ptr(), qd.data_ptr(), tau_seq.data_ptr(), float(dt), int(K), traj.data_ptr(), B,
                      max(ld, B, 1), _stream_ptr(stream, dev)), "rollout_contact_batch")
        return traj

    def contact_wrench_batch_host(self, q, qd, dtype=np.float64):
        """Blocking host form of contact_wrench_batch on numpy arrays -> (fext, cforce)."""
        q, qd = _host_soa((q, qd), self.n, dtype)
        B = q.shape[1]
        fext = np.empty((6 * self.n, B), dtype=q.dtype)
        cforce = np.empty((3 * max(self.n_contacts, 1), B), dtype=q.dtype)
        fn = getattr(_lib, f"multibody_contact_wrench_batch_host_{'f32' if q.dtype == np.float32 else 'f64'}")
        _check(fn(self._h, *[a.ctypes.data for a in (q, qd, fext, cforce)], B), "contact_wrench_batch_host")
        return fext, cforce

    def rollout_contact_batch_host(self, q, qd, tau_seq, dt, dtype=np.float64):
        """Blocking host form of rollout_contact_batch on numpy arrays; tau_seq [K, n, B].  Returns
        (traj [K, n, B], q [n, B], qd [n, B]) -- the inputs are not modified."""
        q, qd = (a.copy() for a in _host_soa((q, qd), self.n, dtype))
        B = q.shape[1]
        tau = np.ascontiguousarray(tau_seq, dtype=q.dtype)
        if tau.ndim != 3 or tau.shape[1:] != (self.n, B):
            raise ValueError(f"tau_seq must be [K, {self.n}, {B}]")
        traj = np.empty_like(tau)
        fn = getattr(_lib, f"multibody_rollout_contact_batch_host_{'f32' if q.dtype == np.float32 else 'f64'}")
        _check(fn(self._h, q.ctypes.data, qd.ctypes.data, tau.ctypes.data, float(dt), tau.shape[0], traj.ctypes.data, B),
               "rollout_contact_batch_host")
        return traj, q, qd

    # ------------------------------------------------------- batched, device [n, B]
    def _soa_call(self, kind, ins, outs, stream):
        """multibody_<kind>_batch_f32 / _f64 on [rows, B] CUDA tensors.  ins: (tensor, name) pairs,
        each [n, B]; the first sets the dtype and B.  outs: (tensor, name, rows) triples: None is
        allocated with the inputs' leading dimension, False is not wanted (passed as NULL), a
        tensor is checked like an input.  Returns the outputs in order (False where skipped)."""
        q = _soa(ins[0][0], self.n, ins[0][1])
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"{ins[0][1]} has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        ts = [q] + [_soa(t, self.n, name, q.dtype, B) for t, name in ins[1:]]
        res = []
        for o, name, rows in outs:
            if o is None:
                o = torch.empty((rows, _ld(q)), dtype=q.dtype, device=q.device)[:, :B]
            elif o is not False:
                _soa(o, rows, name, q.dtype, B)
            res.append(o)
        live = ts + [o for o in res if o is not False]
        ld = _same_ld(live)
        dev = _one_device(live)
        fn = getattr(_lib, f"multibody_{kind}_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, *[t.data_ptr() for t in ts], *[None if o is False else o.data_ptr() for o in res],
                      B, ld, _stream_ptr(stream, dev)), f"{kind}_batch")
        return res

    def rnea_deriv_batch(self, q, qd, qdd, want=("q", "qd"), stream=None):
        """multibody_rnea_deriv_batch_*: the derivatives of tau = rnea(q, qd, qdd) named in `want`
        ("q": d tau / d q, "qd": d tau / d qd), in that order, as [n*n, B] tensors -- row i + n k of
        column b is d tau_i / d q_k of configuration b.  One launch; a matrix not wanted is not
        computed."""
        want = tuple(want)
        if not want or any(w not in ("q", "qd") for w in want) or len(set(want)) != len(want):
            raise ValueError('want must name "q" and / or "qd"')
        outs = self._soa_call("rnea_deriv", [(q, "q"), (qd, "qd"), (qdd, "qdd")],
                              [(None if w in want else False, "dtau_d" + w, self.n * self.n) for w in ("q", "qd")],
                              stream)
        return tuple(outs[("q", "qd").index(w)] for w in want)

    def fd_deriv_batch(self, q, qd, tau, stream=None):
        """multibody_fd_deriv_batch_*: (qdd [n, B], dqdd_dq, dqdd_dqd, dqdd_dtau [n*n, B]) of
        qdd = fd(q, qd, tau) in one launch; qdd is fd_batch's, bit for bit."""
        nn = self.n * self.n
        return tuple(self._soa_call("fd_deriv", [(q, "q"), (qd, "qd"), (tau, "tau")],
                                    [(None, "qdd", self.n), (None, "dqdd_dq", nn), (None, "dqdd_dqd", nn),
                                     (None, "dqdd_dtau", nn)], stream))

    def rnea_batch(self, q, qd, qdd, out=None, stream=None):
        return self._soa_call("rnea", [(q, "q"), (qd, "qd"), (qdd, "qdd")], [(out, "tau", self.n)], stream)[0]

    def fd_batch(self, q, qd, tau, out=None, stream=None):
        return self._soa_call("fd", [(q, "q"), (qd, "qd"), (tau, "tau")], [(out, "qdd", self.n)], stream)[0]

    def rnea_fd_batch(self, q, qd, qdd, tau_in, tau=None, qdd_out=None, stream=None):
        """multibody_rnea_fd_batch_*: (tau = rnea(q, qd, qdd), qdd_out = fd(q, qd, tau_in)) in one
        launch for mass-matrix models (two kernels otherwise); [n, B] CUDA tensors."""
        return tuple(self._soa_call("rnea_fd", [(q, "q"), (qd, "qd"), (qdd, "qdd"), (tau_in, "tau_in")],
                                    [(tau, "tau", self.n), (qdd_out, "qdd_out", self.n)], stream))

    def crba_batch(self, q, out=None, stream=None):
        return self._soa_call("crba", [(q, "q")], [(out, "out", self.n * self.n)], stream)[0]

    def fwd_kin_batch(self, q, out=None, stream=None):
        return self._soa_call("fwd_kin", [(q, "q")], [(out, "out", 3)], stream)[0]

    def jac_batch(self, q, out=None, stream=None):
        return self._soa_call("jac", [(q, "q")], [(out, "out", 6 * self.n)], stream)[0]

    # ---- tiled layout [ceil(B/256), n, 256] (rigidbody_batch.h) ----------------------
    def _tiled(self, t, name, B, rows, dtype=None):
        T = (B + TILE - 1) // TILE
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError(f"{name} must be a CUDA (HIP) torch tensor of shape [tiles, {rows}, 256]")
        if tuple(t.shape) != (T, rows, TILE) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous [{T}, {rows}, {TILE}] tensor for batch {B}")
        if dtype is not None and t.dtype != dtype:
            raise TypeError(f"{name} has dtype {t.dtype}, expected {dtype}")
        return t

    def _tiled_call(self, kind, ins, outs, B, stream):
        """multibody_<kind>_batch_tiled_f32 / _f64: as _soa_call on tiled tensors -- ins
        [ceil(B/256), n, 256], outs (tensor or None, name, rows) [ceil(B/256), rows, 256]."""
        q = self._tiled(ins[0][0], ins[0][1], B, self.n)
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"{ins[0][1]} has dtype {q.dtype}, expected float32 or float64")
        ts = [q] + [self._tiled(t, name, B, self.n, q.dtype) for t, name in ins[1:]]
        res = [torch.empty((q.shape[0], rows, TILE), dtype=q.dtype, device=q.device) if o is None
               else self._tiled(o, name, B, rows, q.dtype) for o, name, rows in outs]
        dev = _one_device(ts + res)
        fn = getattr(_lib, f"multibody_{kind}_batch_tiled_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, *[t.data_ptr() for t in ts + res], B, _stream_ptr(stream, dev)), f"{kind}_batch_tiled")
        return res

    def rnea_batch_tiled(self, q, qd, qdd, B, out=None, stream=None):
        """RNEA on tiled [ceil(B/256), n, 256] tensors (see to_tiled)."""
        return self._tiled_call("rnea", [(q, "q"), (qd, "qd"), (qdd, "qdd")], [(out, "out", self.n)], B, stream)[0]

    def fd_batch_tiled(self, q, qd, tau, B, out=None, stream=None):
        return self._tiled_call("fd", [(q, "q"), (qd, "qd"), (tau, "tau")], [(out, "out", self.n)], B, stream)[0]

    def rnea_fd_batch_tiled(self, q, qd, qdd, tau_in, B, tau=None, qdd_out=None, stream=None):
        """rnea_fd_batch on tiled [ceil(B/256), n, 256] tensors (multibody_rnea_fd_batch_tiled_*)."""
        return tuple(self._tiled_call("rnea_fd", [(q, "q"), (qd, "qd"), (qdd, "qdd"), (tau_in, "tau_in")],
                                      [(tau, "tau", self.n), (qdd_out, "qdd_out", self.n)], B, stream))

    def crba_batch_tiled(self, q, B, out=None, stream=None):
        """Mass matrices on the tiled layout: q [ceil(B/256), n, 256] -> [ceil(B/256), n*n, 256]."""
        return self._tiled_call("crba", [(q, "q")], [(out, "out", self.n * self.n)], B, stream)[0]

    def fwd_kin_batch_tiled(self, q, B, out=None, stream=None):
        return self._tiled_call("fwd_kin", [(q, "q")], [(out, "out", 3)], B, stream)[0]

    def jac_batch_tiled(self, q, B, out=None, stream=None):
        return self._tiled_call("jac", [(q, "q")], [(out, "out", 6 * self.n)], B, stream)[0]

    def rollout_batch(self, q, qd, tau_seq, dt, traj=False, stream=None):
        """K fused forward-dynamics + semi-implicit Euler steps, in place on q and qd
        ([n, B] CUDA tensors); tau_seq [K, n, B].  Returns the trajectory [K, n, B] of q
        when traj=True (else None)."""
        q = _soa(q, self.n, "q")
        B = q.shape[1]
        qd = _soa(qd, self.n, "qd", q.dtype, B)
        if not isinstance(tau_seq, torch.Tensor) or tau_seq.dim() != 3 or tau_seq.shape[1:] != (self.n, B):
            raise ValueError(f"tau_seq must be [K, {self.n}, {B}]")
        if tau_seq.dtype != q.dtype or not tau_seq.is_contiguous():
            raise ValueError("tau_seq must be contiguous with the state's dtype")
        ld = _same_ld((q, qd))
        if B > 1 and ld != B:
            raise ValueError("rollout needs contiguous [n, B] state (ld == B), like tau_seq")
        K = tau_seq.shape[0]
        tr = torch.empty_like(tau_seq) if traj else None
        dev = _one_device((q, qd, tau_seq))
        fn = getattr(_lib, f"multibody_rollout_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, q.data_ptr(), qd.data_ptr(), tau_seq.data_ptr(), float(dt), int(K),
                      tr.data_ptr() if tr is not None else None, B, max(ld, B, 1), _stream_ptr(stream, dev)),
                   "rollout_batch")
        return tr

    def rollout_vjp_batch(self, q, qd, tau_seq, dt, gq, gqd, stream=None, _op="rollout_vjp"):
        """multibody_rollout_vjp_batch_*: the reverse-mode gradient of rollout_batch in one launch.
        q, qd [n, B] (the initial state, not modified), tau_seq [K, n, B]; gq, gqd [K, n, B] are the
        cotangents of the state after step k (gq[k] pairs with traj[k], gqd[K-1] with the final qd).
        Returns (g_q0 [n, B], g_qd0 [n, B], g_tau [K, n, B]).  The [K, 2n, B] workspace is allocated
        here.  Every array is contiguous (ld == B), like the rollout's."""
        q = _soa(q, self.n, "q")
        if q.dtype not in _TORCH_SUFFIX:
            raise TypeError(f"q has dtype {q.dtype}, expected float32 or float64")
        B = q.shape[1]
        qd = _soa(qd, self.n, "qd", q.dtype, B)
        ld = _same_ld((q, qd))
        if B > 1 and ld != B:
            raise ValueError("rollout_vjp needs contiguous [n, B] state (ld == B), like tau_seq")
        if not isinstance(tau_seq, torch.Tensor) or tau_seq.dim() != 3 or tau_seq.shape[1:] != (self.n, B):
            raise ValueError(f"tau_seq must be [K, {self.n}, {B}]")
        K = tau_seq.shape[0]
        for t, name in ((tau_seq, "tau_seq"), (gq, "gq"), (gqd, "gqd")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (K, self.n, B):
                raise ValueError(f"{name} must be [{K}, {self.n}, {B}]")
            if t.dtype != q.dtype or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous with the state's dtype")
        dev = _one_device((q, qd, tau_seq, gq, gqd))
        g_q0, g_qd0, g_tau = torch.empty_like(q), torch.empty_like(qd), torch.empty_like(tau_seq)
        work = torch.empty((K, 2 * self.n, B), dtype=q.dtype, device=dev)
        fn = getattr(_lib, f"multibody_{_op}_batch_{_TORCH_SUFFIX[q.dtype]}")
        with torch.cuda.device(dev):
            _check(fn(self._h, q.data_ptr(), qd.data_ptr(), tau_seq.data_ptr(), float(dt), int(K), gq.data_ptr(),
                      gqd.data_ptr(), g_q0.data_ptr(), g_qd0.data_ptr(), g_tau.data_ptr(), work.data_ptr(), B,
                      max(ld, B, 1), _stream_ptr(stream, dev)), f"{_op}_batch")
        return g_q0, g_qd0, g_tau

    def rollout_contact_vjp_batch(self, q, qd, tau_seq, dt, gq, gqd, stream=None):
        """multibody_rollout_contact_vjp_batch_*: rollout_vjp_batch through rollout_contact_batch -- the
        reverse-mode gradient of the fused contact rollout in one launch, the same arrays."""
        return self.rollout_vjp_batch(q, qd, tau_seq, dt, gq, gqd, stream, _op="rollout_contact_vjp")

    # -------------------------------------------------------- batched, host [n, B]
    def rollout_vjp_batch_host(self, q, qd, tau_seq, dt, gq, gqd, dtype=np.float64, _op="rollout_vjp"):
        """Blocking host form of rollout_vjp_batch on numpy arrays: q, qd [n, B]; tau_seq, gq, gqd
        [K, n, B].  Returns (g_q0, g_qd0 [n, B], g_tau [K, n, B])."""
        q, qd = _host_soa((q, qd), self.n, dtype)
        B = q.shape[1]
        seqs = [np.ascontiguousarray(x, dtype=q.dtype) for x in (tau_seq, gq, gqd)]
        K = seqs[0].shape[0] if seqs[0].ndim == 3 else -1
        for a in seqs:
            if a.shape != (K, self.n, B):
                raise ValueError(f"tau_seq, gq and gqd must all be [K, {self.n}, {B}], got {a.shape}")
        outs = [np.empty_like(q), np.empty_like(q), np.empty_like(seqs[0])]
        fn = getattr(_lib, f"multibody_{_op}_batch_host_{'f32' if q.dtype == np.float32 else 'f64'}")
        _check(fn(self._h, q.ctypes.data, qd.ctypes.data, seqs[0].ctypes.data, float(dt), K,
                  *[a.ctypes.data for a in (seqs[1], seqs[2], *outs)], B), f"{_op}_batch_host")
        return tuple(outs)

    def rollout_contact_vjp_batch_host(self, q, qd, tau_seq, dt, gq, gqd, dtype=np.float64):
        """Blocking host form of rollout_contact_vjp_batch on numpy arrays, as rollout_vjp_batch_host."""
        return self.rollout_vjp_batch_host(q, qd, tau_seq, dt, gq, gqd, dtype, _op="rollout_contact_vjp")

    def _host_call(self, kind, ins, out_rows, dtype):
        """multibody_<kind>_batch_host_f64 / _f32 (blocking): `ins` as [n, B] numpy arrays of
        `dtype`; returns one new [rows, B] array per entry of out_rows."""
        arrs = _host_soa(ins, self.n, dtype)
        B = arrs[0].shape[1]
        outs = [np.empty((rows, B), dtype=arrs[0].dtype) for rows in out_rows]
        fn = getattr(_lib, f"multibody_{kind}_batch_host_{'f32' if arrs[0].dtype == np.float32 else 'f64'}")
        _check(fn(self._h, *[a.ctypes.data for a in arrs + outs], B), f"{kind}_batch_host")
        return outs

    def rnea_batch_host(self, q, qd, qdd, dtype=np.float64):
        """Blocking host form: multibody_rnea_batch_host_f64 (default: fp64, the reference's Real,
        whatever the inputs' dtype) or _f32 with dtype=np.float32."""
        return self._host_call("rnea", (q, qd, qdd), [self.n], dtype)[0]

    def fd_batch_host(self, q, qd, tau, dtype=np.float64):
        """Blocking host form: multibody_fd_batch_host_f64 (default) or _f32 (dtype=np.float32)."""
        return self._host_call("fd", (q, qd, tau), [self.n], dtype)[0]

    def rnea_fd_batch_host(self, q, qd, qdd, tau_in, dtype=np.float64):
        """Blocking host form of rnea_fd_batch: (tau, qdd_out) as [n, B] numpy arrays
        (multibody_rnea_fd_batch_host_f64, or _f32 with dtype=np.float32)."""
        return tuple(self._host_call("rnea_fd", (q, qd, qdd, tau_in), [self.n] * 2, dtype))

    def rnea_deriv_batch_host(self, q, qd, qdd, dtype=np.float64):
        """Blocking host form of rnea_deriv_batch: (dtau_dq, dtau_dqd) as [n*n, B] numpy arrays."""
        return tuple(self._host_call("rnea_deriv", (q, qd, qdd), [self.n * self.n] * 2, dtype))

    def fd_deriv_batch_host(self, q, qd, tau, dtype=np.float64):
        """Blocking host form of fd_deriv_batch: (qdd [n, B], dqdd_dq, dqdd_dqd, dqdd_dtau [n*n, B])."""
        return tuple(self._host_call("fd_deriv", (q, qd, tau), [self.n] + [self.n * self.n] * 3, dtype))


def to_tiled(x, stream=None):
    """[rows, B] SoA CUDA tensor -> new [ceil(B/256), rows, 256] tiled tensor (rb_to_tiled_*)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise TypeError("to_tiled needs a CUDA tensor [rows, B] contiguous along B")
    rows, B = x.shape
    out = torch.empty(((B + TILE - 1) // TILE, rows, TILE), dtype=x.dtype, device=x.device)
    fn = getattr(_lib, f"rb_to_tiled_{_TORCH_SUFFIX[x.dtype]}")
    with torch.cuda.device(x.device):
        _check(fn(x.data_ptr(), _ld(x), out.data_ptr(), rows, B, _stream_ptr(stream, x.device)), "to_tiled")
    return out


def from_tiled(t, B, stream=None):
    """[ceil(B/256), rows, 256] tiled tensor -> new [rows, B] SoA tensor (rb_from_tiled_*)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 3 or t.shape[2] != TILE or \
            t.shape[0] != (B + TILE - 1) // TILE or not t.is_contiguous():
        raise TypeError(f"from_tiled needs a contiguous CUDA tensor [ceil(B/256), rows, 256] for B={B}")
    rows = t.shape[1]
    out = torch.empty((rows, B), dtype=t.dtype, device=t.device)
    fn = getattr(_lib, f"rb_from_tiled_{_TORCH_SUFFIX[t.dtype]}")
    with torch.cuda.device(t.device):
        _check(fn(t.data_ptr(), out.data_ptr(), max(B, 1), rows, B, _stream_ptr(stream, t.device)), "from_tiled")
    return out


def fill_uniform(t, lo, hi, seed, stream=None):
    """rb_fill_uniform_*: t[j, b] = lo[j] + (hi[j]-lo[j]) * u(seed, j, b) on the device."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise TypeError("fill_uniform needs a CUDA tensor [rows, B] contiguous along B")
    rows, B = t.shape
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    if lo.shape != (rows,) or hi.shape != (rows,):
        raise ValueError("lo/hi must have one value per row")
    fn = getattr(_lib, f"rb_fill_uniform_{_TORCH_SUFFIX[t.dtype]}")
    with torch.cuda.device(t.device):
        _check(fn(t.data_ptr(), rows, B, _ld(t), lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp),
                  ctypes.c_uint64(seed), _stream_ptr(stream, t.device)), "fill_uniform")
    return t
