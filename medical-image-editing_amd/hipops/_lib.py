"""ctypes binding of libvqwnet_hip.so (the C ABI declared in include/vqwnet_hip.h).

The prototypes and the ABI version are read from the header itself, which the compiler checks every entry point's
definition against, so the binding cannot drift from the library.

The library is built in-tree by `make -C medical-image-editing_amd/csrc` (or
__graft_entry__.build()).  There is NO fallback: if the shared object is missing
every operator raises — the product path never routes through PyTorch eager
kernels or the CPU oracle.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VQW_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libvqwnet_hip.so")   # override: A/B of two builds

HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "vqwnet_hip.h")

_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}


def _ctype(ctype, name, ret=False):
    """ctypes type of a C parameter type (any pointer -> c_void_p) or return type (`const char*` -> c_char_p)."""
    if ctype.endswith("*"):
        if not ret:
            return ctypes.c_void_p
        if ctype == "const char*":
            return ctypes.c_char_p
    elif ctype in _SCALARS:
        return _SCALARS[ctype]
    raise RuntimeError("%s: no ctypes type for the C type %r" % (name, ctype))


def parse_header(path=HEADER):
    """-> {name: (return C type, [(kind, name, C type)])} with kind in {'in', 'out', 'int', 'float', 'stream', 'host'}."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"(//|^\s*#)[^\n]*", " ", text, flags=re.M)       # comments, preprocessor lines
    protos = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(vqw_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, name, params = re.sub(r"\s*\*", "*", " ".join(m.group(1).split())), m.group(2), m.group(3).strip()
        args = []
        if params and params != "void":
            for p in params.split(","):
                p = re.sub(r"\s*\*\s*", "* ", " ".join(p.split()))
                pname = re.findall(r"\w+", p)[-1]
                ctype = p[:p.rindex(pname)].strip()
                if "*" in p:
                    if pname == "stream":
                        kind = "stream"
                    elif name.endswith("_host"):
                        kind = "host"                 # host arrays passed by value (vqw_weighted_sum_host)
                    else:
                        kind = "in" if p.startswith("const ") else "out"
                else:
                    ctype = ctype.replace("const ", "")
                    _ctype(ctype, name)
                    kind = "float" if ctype in ("float", "double") else "int"
                args.append((kind, pname, ctype))
        protos[name] = (ret, args)
    return protos


def signatures(path=HEADER):
    """-> {name: (restype, argtypes)}: the ctypes prototypes of the header's functions."""
    return {name: (_ctype(ret, name, ret=True), [_ctype(t, name) for _, _, t in args])
            for name, (ret, args) in parse_header(path).items()}


SIGNATURES = signatures()
ABI_VERSION = int(re.search(r"(?m)^\s*#\s*define\s+VQW_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))

_lib = None


def load():
    """Load (once) and return the CDLL with prototypes set.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libvqwnet_hip.so is not built (%s). Run `make -C medical-image-editing_amd/csrc` "
            "or __graft_entry__.build(); there is no CPU/eager fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the header and the library diverge
        fn.restype = res
        fn.argtypes = args
    if lib.vqw_abi_version() != ABI_VERSION:
        raise RuntimeError("libvqwnet_hip.so has ABI %d, the host code expects %d: rebuild it (make -C medical-image-editing_amd/csrc)"
                           % (lib.vqw_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(status, name="vqw"):
    if status != 0:
        msg = load().vqw_last_error()
        raise RuntimeError("%s failed (%d): %s" % (name, status, (msg or b"").decode()))
