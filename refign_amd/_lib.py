"""ctypes binding of librefign_hip.so (C ABI: include/refign_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C refign_amd/csrc` into refign_amd/lib/.
Loading is lazy and LOUD: if the .so is missing or does not export a declared symbol we raise -- the product path
never falls back to a CPU or PyTorch implementation.
"""
import ctypes
import os
import re
import threading

from ._tensor import current_stream, on_device

_HERE = os.path.dirname(os.path.abspath(__file__))
# (RFN_LIB: another build of the same library, for A/B runs of kernel variants -- tools/ab_build.sh)
_LIB_PATH = os.environ.get("RFN_LIB") or os.path.join(_HERE, "lib", "librefign_hip.so")
_lock = threading.Lock()
_lib = None

c_void_p = ctypes.c_void_p
_HEADER = os.path.join(_HERE, os.pardir, "include", "refign_hip.h")
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "unsigned long": ctypes.c_ulong, "float": ctypes.c_float,
            "double": ctypes.c_double, "rfn_stream_t": c_void_p}


def parse_header(text):
    """(RFN_ABI_VERSION, {name: (restype, argtypes)}) of a C-ABI header: every `ret rfn_name(args);` it declares.  Any
    pointer and rfn_stream_t become c_void_p (a `const char*` RETURN: c_char_p), scalars map through _SCALARS; a type
    that is in neither raises and names the declaration -- never guessed."""
    version = int(re.search(r"^\s*#\s*define\s+RFN_ABI_VERSION\s+(\d+)", text, re.M).group(1))
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*", " ", text, flags=re.S | re.M)

    def ctype(decl, what, is_return=False):
        words = [w for w in decl.replace("*", " * ").split() if w != "const"]
        if "*" in words:
            return ctypes.c_char_p if is_return and words == ["char", "*"] else c_void_p
        key = " ".join(words if is_return else words[:-1])      # a by-value parameter carries its name
        if key not in _SCALARS or (not is_return and words[-1] in _SCALARS):
            raise ValueError(f"refign_hip.h: unknown C type in `{decl.strip()}` of {what}")
        return _SCALARS[key]

    signatures = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(rfn_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [] if args.strip() in ("", "void") else args.split(",")
        signatures[name] = (ctype(ret, name, True), [ctype(a, name) for a in args])
    return version, signatures


with open(_HEADER) as _f:
    ABI_VERSION, SIGNATURES = parse_header(_f.read())


def library_path():
    return _LIB_PATH


def load_library():
    """Load librefign_hip.so and bind every declared entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"refign_amd: HIP library not built: {_LIB_PATH} is missing. Run `python -c 'import "
                f"__graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # torch owns device memory and streams; import it FIRST so that its bundled libamdhip64.so.7 is the one HIP
        # runtime in the process (our .so NEEDs the same SONAME and binds to the already-loaded copy).  Loading ours
        # first would pull /opt/rocm's runtime in beside torch's: two runtimes, "no ROCm-capable device" at launch.
        import torch  # noqa: F401
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise RuntimeError(f"refign_amd: {_LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if lib.rfn_abi_version() != ABI_VERSION:
            raise RuntimeError(f"refign_amd: {_LIB_PATH} speaks ABI {lib.rfn_abi_version()}, this package binds ABI {ABI_VERSION} "
                               f"(include/refign_hip.h: RFN_ABI_VERSION): rebuild the library")
        _lib = lib
    return _lib


def abi_version():
    return load_library().rfn_abi_version()


def check(rc, what):
    """Turn a non-zero ABI return code into RuntimeError (what TORCH_CHECK raises in the reference)."""
    if rc != 0:
        msg = load_library().rfn_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def call(name, device, *args):
    """Launch entry point `name` on `device`: on torch's current stream there (every launching entry point takes the
    stream LAST), RuntimeError on a non-zero code.  The one place the launch protocol lives: ~3 000 calls per eager step."""
    with on_device(device):
        rc = getattr(_lib or load_library(), name)(*args, current_stream(device))
    if rc != 0:
        check(rc, name)
