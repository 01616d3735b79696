"""ctypes binding of ``libplanedepth_hip.so`` (C ABI declared in ``include/planedepth_hip.h``).

There is deliberately NO fallback: if the shared library is missing or a symbol is absent, importing the product
ops raises.  The library is built in-tree by ``__graft_entry__.build()`` (``hipcc --offload-arch=gfx950``).

The header is the one declaration of the boundary: the prototypes (``SIGNATURES``) and the ``PD_*`` constants are read from
it when this module is imported, and the three struct mirrors below are compared with its members.  Adding an entry point
means declaring it in the header and defining it; nothing is repeated here.  Launches go through ``call``.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (imported first so the process already holds torch's libamdhip64 — one HIP runtime only)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PD_LIB") or os.path.join(_HERE, "lib", "libplanedepth_hip.so")  # PD_LIB: diagnostics builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "planedepth_hip.h")   # the one declaration of the C boundary


class SweepDesc(ctypes.Structure):
    """Mirror of ``pd_sweep_desc``."""
    _fields_ = [("B", ctypes.c_int32), ("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("flags", ctypes.c_int32), ("sign", ctypes.c_float),
                ("impl", ctypes.c_int32)]


class SweepView(ctypes.Structure):
    """Mirror of ``pd_sweep_view``: what differs between two target views of one source image (pd_uniform_*_pair)."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "tgt", "plane", "plane_aux", "inv_K3", "padding_mask", "dists", "rgb_rec", "ph_map", "ph_mean", "stash",
        "g_rgb_rec", "g_ph_map", "g_ph_mean", "g_plane", "g_dists", "workspace")]


def sweep_view(**tensors):
    """SweepView from keyword tensors (missing / None -> NULL)."""
    v = SweepView()
    for name, t in tensors.items():
        setattr(v, name, None if t is None else t.data_ptr())
    return v


class PpRoute(ctypes.Structure):
    """Mirror of ``pd_pp_route``: the kernel a post-process call is served by (pd_warp_route / pd_post_process_route)."""
    _fields_ = [("family", ctypes.c_int32), ("flip", ctypes.c_int32), ("nmax", ctypes.c_int32), ("rows2", ctypes.c_int32),
                ("alias", ctypes.c_int32), ("lds_bytes", ctypes.c_uint32)]


class PlaneDepthHipError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int32_t": ctypes.c_int32,
            "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "pd_stream_t": ctypes.c_void_p}
_DATA = ("void", "float", "int", "int32_t", "int64_t", "uint8_t")   # pointees of a data pointer: c_void_p
_MIRRORS = {"pd_sweep_desc": SweepDesc, "pd_sweep_view": SweepView, "pd_pp_route": PpRoute}


def _ctype(text, decl, result=False):
    """The ctypes type of one parameter (or of the result) of ``decl``; a type outside the header's vocabulary raises."""
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*\w*", text.strip())
    base, star = m.groups() if m else (None, None)
    if not star and base in _SCALARS:
        return _SCALARS[base]
    if star and base in _MIRRORS:
        return ctypes.POINTER(_MIRRORS[base])
    if star and base in _DATA and not result:
        return ctypes.c_void_p
    if star and base == "char" and result:
        return ctypes.c_char_p
    raise PlaneDepthHipError("%s: no ctypes mapping for `%s` in `%s`" % (HEADER_PATH, text.strip(), decl))


def _parse_header():
    """(constants, prototypes) of the header: every ``PD_X = n`` of every enum, and name -> (restype, argtypes) for every
    ``ret pd_name(params);``.  The struct mirrors are compared with the header's members on the way."""
    try:
        with open(HEADER_PATH) as f:
            text = f.read()
    except OSError as e:
        raise PlaneDepthHipError("planedepth_amd: cannot read the C header %s (%s); the prototypes and constants are derived "
                                 "from it and there is no fallback table" % (HEADER_PATH, e))
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*", " ", text, flags=re.S | re.M)   # comments, preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    constants, members = {}, {}

    def enum(m):
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            kv = re.fullmatch(r"(PD_\w+)\s*=\s*(-?\d+)", item)
            if not kv:
                raise PlaneDepthHipError("%s: cannot read the enum value `%s` (decimal literals only)" % (HEADER_PATH, item))
            constants[kv.group(1)] = int(kv.group(2))
        return ""

    def struct(m):
        members[m.group(1)] = re.findall(r"(\w+)\s*[,;]", m.group(2))
        return ""
    text = re.sub(r"\benum\b\s*\w*\s*\{([^}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*\1\s*;", struct, text)
    text = re.sub(r"\btypedef\s+void\s*\*\s*pd_stream_t\s*;", "", text)
    for c_name, mirror in _MIRRORS.items():
        if members.get(c_name) != [f[0] for f in mirror._fields_]:
            raise PlaneDepthHipError("%s: %s has the members %s, its mirror %s has %s" % (
                HEADER_PATH, c_name, members.get(c_name), mirror.__name__, [f[0] for f in mirror._fields_]))
    prototypes = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(pd_\w+) ?\(([^()]*)\)", decl)
        if not m:
            raise PlaneDepthHipError("%s: cannot read the declaration `%s`" % (HEADER_PATH, decl))
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        prototypes[name] = (_ctype(ret, decl, result=True), [_ctype(p, decl) for p in params])
    return constants, prototypes


# Everything the header declares, derived from it: the PD_* enum values as module attributes, and
# SIGNATURES: name -> (restype, argtypes).  A new entry point is declared in the header and defined; nothing is added here.
_CONSTANTS, SIGNATURES = _parse_header()
globals().update(_CONSTANTS)
PD_PP_FAMILIES = tuple(k[len("PD_PP_FAMILY_"):].lower()   # pd_pp_family, by value
                       for k in sorted((k for k in _CONSTANTS if k.startswith("PD_PP_FAMILY_")), key=_CONSTANTS.get))

_lib = None


def bind(lib):
    """Attach the header's prototypes to a loaded library (``load`` does; so do scripts that side-load another build)."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load the library once and attach prototypes.  Raises if it is missing — never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise PlaneDepthHipError(
            "planedepth_amd: %s not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for the hot path." % LIB_PATH)
    _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().pd_last_error().decode(errors="replace")
        raise PlaneDepthHipError("%s failed (code %d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


POISON_LDS = bool(int(os.environ.get("PD_DEBUG_POISON_LDS", "0")))   # diagnostics: NaNs into the CUs' LDS before every launch


class _NoSwitch:
    """`with` target that does nothing (the tensor's device already is the current one)."""
    __slots__ = ()

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def on_device(device):
    """`with on_device(t.device):` — torch.cuda.device(device) only when a switch is needed.  The context manager costs
    several microseconds per entry (two set_device calls and their bookkeeping), which is most of what the HOST spends on
    an operator whose kernels take 30 us; on a one-GPU-per-process layout the tensor's device always is the current one."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(device)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # (absent from some torch builds: the Stream object then)


def raw_stream(device=None):
    """torch's current stream on ``device`` as an integer (the hipStream_t).  torch.cuda.current_stream() builds a Stream object
    per call — ~10 us, four times per training step here (two launches, two pool look-ups: 40 of the step's 214 us of host time);
    the raw getter is a plain C call."""
    if _RAW_STREAM is not None:
        if device is None or isinstance(device, int):
            idx = device
        else:
            idx = (device if isinstance(device, torch.device) else torch.device(device)).index
        return _RAW_STREAM(torch.cuda.current_device() if idx is None else int(idx))
    return torch.cuda.current_stream(device).cuda_stream


def stream_handle(device=None):
    """The raw hipStream_t torch is currently enqueueing on (so our launches order with torch's ops)."""
    h = ctypes.c_void_p(raw_stream(device))
    if POISON_LDS:   # a kernel that reads shared memory it never wrote then produces NaNs instead of luck
        load().pd_debug_poison_lds(h)
    return h


def call(name, device, *args):
    """Launch the stream-taking entry point ``name`` on torch's current stream of ``device``: ``args`` are the header's
    parameters without the trailing ``pd_stream_t``.  A tensor passes its ``data_ptr()``, None is NULL, everything else
    (numbers, ``byref(...)``, ctypes arrays) goes through as it is.  A wrong argument count is a TypeError before anything
    touches the device; a refusal by the library raises PlaneDepthHipError with its message.  Contiguity, dtypes and
    keeping temporaries alive until the launch are the caller's business."""
    fn = getattr(load(), name)
    if len(args) + 1 != len(fn.argtypes):
        raise TypeError("%s takes %d arguments before its stream, got %d" % (name, len(fn.argtypes) - 1, len(args)))
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    with on_device(device):
        rc = fn(*args, stream_handle(device))
    if rc:
        check(rc, name)


def require_gpu_tensor(name, t, shape=None, dtype=torch.float32):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise PlaneDepthHipError("%s is on %s: planedepth_amd runs on the GPU only (no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t
