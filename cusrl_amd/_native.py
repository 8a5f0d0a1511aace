"""ctypes binding of ``libcusrl_hip.so`` (C ABI declared in ``include/cusrl_hip.h``).

The library is the product: there is no CPU or eager fallback.  If it has not been built
(``python __graft_entry__.py`` / ``__graft_entry__.build()``) every hot-path call raises.
"""

from __future__ import annotations

import ctypes
import re
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p
from pathlib import Path

from cusrl_amd.utils import switches

# (another build of the same library: A/B runs of compile-time variants, profiles/r05/loss_variants_ab.txt)
LIB_PATH = Path(switches.read("HIP_LIBRARY") or Path(__file__).resolve().parent / "libcusrl_hip.so")


class Field(Structure):
    """``cusrl_field_t`` — one buffer leaf of a multi-leaf launch."""

    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("row_bytes", c_int64)]


class PackedField(Structure):
    """``cusrl_packed_field_t`` — one narrow leaf's place inside the per-slot record."""

    _fields_ = [("ptr", c_void_p), ("offset", ctypes.c_int32), ("width", ctypes.c_int32)]


class GradPiece(Structure):
    """``cusrl_grad_piece_t`` — one parameter's slot of the flat gradient buffer and what to sum into it."""

    _fields_ = [("src", c_void_p), ("offset", c_int64), ("numel", c_int64), ("splits", c_int64), ("row_stride", c_int64)]


class MirrorField(Structure):
    """``cusrl_mirror_field_t`` — one field of a ``cusrl_mirror_rows`` launch (a copy, or the mirror through a table)."""

    _fields_ = [("src", c_void_p), ("src_stride", c_int64), ("dst", c_void_p), ("dst_stride", c_int64), ("dst_offset", c_int64),
                ("table", c_void_p), ("width", ctypes.c_int32), ("src_width", ctypes.c_int32)]


class NativeError(RuntimeError):
    pass


_lib = None

# The binding is READ from the header, not copied from it: `ret name(args);` for every prototype and the `#define`d integer
# constants of include/cusrl_hip.h, in the header's own restricted C.  The mapping is fixed; a declaration outside it is an error.
HEADER_PATH = Path(__file__).resolve().parent.parent / "include" / "cusrl_hip.h"
_SCALARS = {"int": c_int, "int32_t": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float, "double": c_double}
_STRUCTS = {"cusrl_field_t": Field, "cusrl_packed_field_t": PackedField, "cusrl_grad_piece_t": GradPiece,
            "cusrl_mirror_field_t": MirrorField}
_POINTEES = {"void", "char", "float", "double", "int", "uint8_t", "int32_t", "uint32_t", "int64_t", "uint64_t"}


def _ctype(declaration: str, where: str, opaque: frozenset = frozenset()):
    """ctypes type of one C declaration (``const float *x``, ``int64_t n``, a bare return type); ``opaque``: names the header
    declares as incomplete struct types.  Pointers other than strings and the registered structs are addresses."""
    words = [word for word in re.findall(r"\w+|\*", declaration) if word != "const"]
    base, stars = (words[0] if words else ""), words.count("*")
    if stars == 0 and base in _SCALARS and len(words) <= 2:
        return _SCALARS[base]
    if len(words) <= stars + 2 and words[1 : stars + 1] == ["*"] * stars:
        if stars == 1 and base == "char":
            return c_char_p
        if stars == 1 and base in _STRUCTS:
            return POINTER(_STRUCTS[base])
        if stars >= 1 and (base in _POINTEES or base in opaque):
            return c_void_p
    raise NativeError(f"{HEADER_PATH.name}: no ctypes mapping for '{declaration.strip()}' in '{where.strip()}'")


def parse_header(text: str) -> tuple[dict[str, int], dict[str, tuple]]:
    """``({constant: value}, {symbol: (restype, argtypes)})`` of a header in the style of include/cusrl_hip.h."""
    constants = {name: int(value) for name, value in re.findall(r"^#define\s+CUSRL_(\w+)\s+\(?(-?\d+)\)?", text, re.M)}
    text = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.M)
    statements = [" ".join(part.split()) for part in re.split(r"[;{}]", text)]
    opaque = frozenset(m.group(1) for m in map(re.compile(r"typedef struct \w+ (\w+)").fullmatch, statements) if m)
    prototypes = {}
    for statement in statements:
        if "(" not in statement:
            continue
        match = re.fullmatch(r"([\w\s*]+?)(\w+) ?\(([^()]*)\)", statement)
        if match is None:
            raise NativeError(f"{HEADER_PATH.name}: not a prototype of the form `ret name(args)`: '{statement}'")
        ret, name, args = match.groups()
        arguments = [] if args.strip() == "void" else args.split(",")
        prototypes[name] = (_ctype(ret, statement, opaque), [_ctype(arg, statement, opaque) for arg in arguments])
    return constants, prototypes


# (read here and not on the first lib(): ABI_VERSION, the MAX_* and EXPORTED_SYMBOLS are attributes of this module)
try:
    _CONSTANTS, _PROTOTYPES = parse_header(HEADER_PATH.read_text())
except OSError as error:
    raise NativeError(f"{HEADER_PATH} cannot be read ({error}): the ctypes binding is derived from it") from error
ABI_VERSION = _CONSTANTS["ABI_VERSION"]
MAX_FIELDS = _CONSTANTS["MAX_FIELDS"]
MAX_PACKED = _CONSTANTS["MAX_PACKED"]
MAX_MIRROR_FIELDS = _CONSTANTS["MAX_MIRROR_FIELDS"]
MAX_SYMMETRIZE_CHANNELS = _CONSTANTS["MAX_SYMMETRIZE_CHANNELS"]
MAX_SYMMETRIC_HEAD_ACTIONS = _CONSTANTS["MAX_SYMMETRIC_HEAD_ACTIONS"]
MAX_LAYER_NORM_WIDTH = _CONSTANTS["MAX_LAYER_NORM_WIDTH"]
MAX_DWCONV_TAPS = _CONSTANTS["MAX_DWCONV_TAPS"]
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)


def lib() -> ctypes.CDLL:
    """Load the HIP library once; fail loudly when it is missing or stale."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise NativeError(
                f"{LIB_PATH} is missing: the gfx950 HIP extension has not been built. "
                "Run `python __graft_entry__.py` (or `__graft_entry__.build()`) first; "
                "cusrl_amd has no CPU / eager fallback for the rollout + PPO-update hot path."
            )
        handle = ctypes.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(handle, name)  # AttributeError here = stale library
            fn.restype = restype
            fn.argtypes = argtypes
        if handle.cusrl_abi_version() != ABI_VERSION:
            raise NativeError(f"ABI mismatch: library {handle.cusrl_abi_version()}, binding {ABI_VERSION}; rebuild")
        _lib = handle
        _options_from_environment()
    return _lib


# The A/B scripts of rounds 2-5 drive the kernels' launch-shape / cache-policy overrides through CUSRL_* environment variables.
# The library no longer reads the environment in its launch entry points (cusrl_set_option, ABI 6): the HOST translates them,
# once, when it loads the library.  {switch: (option,)} — the option's name first, as before; utils/switches.py maps each one's
# text to the option's value.
_ENVIRONMENT_OPTIONS = {
    "GAE_POLICY": ("gae_policy",), "GAE_BLOCK": ("gae_block",), "LOSS_POLICY": ("loss_policy",), "PUSH_POLICY": ("push_policy",),
    "COLSUM_ROWS": ("colsum_rows",), "HEAD_ROWS": ("head_rows",), "GRU_BIAS_ROWS": ("gru_bias_rows",),
}


def set_option(key: str, value: int) -> None:
    """``cusrl_set_option``: force a kernel's launch shape / cache policy (0: back to its own rule); include/cusrl_hip.h."""
    check(lib().cusrl_set_option(key.encode(), int(value)), f"cusrl_set_option({key!r}, {value})")


def get_option(key: str) -> int:
    value = c_int64()
    check(lib().cusrl_get_option(key.encode(), ctypes.byref(value)), f"cusrl_get_option({key!r})")
    return int(value.value)


def _options_from_environment() -> None:
    for switch, (option,) in _ENVIRONMENT_OPTIONS.items():
        value = switches.read(switch)
        if value is not None:
            _lib.cusrl_set_option(option.encode(), value)  # (a value the library refuses leaves the kernel's own rule, too)


# Launch census: how often each C-ABI entry point was called through ``check`` (every ``ops`` function reports its
# launch here).  Tests use it to prove that a result came from the HIP kernel and not from a torch-op form
# (``launch_counts["cusrl_rnd_reward"]`` must move when the RND hook runs on a GPU).
launch_counts: dict[str, int] = {}


def check(code: int, what, arguments: tuple | None = None) -> None:
    """Two ways in.  ``check(status, "cusrl_x")``: count the call under that name and raise on a non-zero status.  As a ctypes
    ``errcheck``, ``check(status, function, arguments)``: ctypes passes the library function and the (always non-None) argument
    tuple; the call is counted under the function's symbol name.  The call then returns None."""
    if arguments is not None:
        what = what.__name__
    launch_counts[what] = launch_counts.get(what, 0) + 1
    if code != 0:
        text = lib().cusrl_error_string(code).decode()
        if code == -4:  # CUSRL_E_COMM
            text += ": " + lib().cusrl_comm_last_error().decode()
        raise NativeError(f"{what} failed with code {code}: {text}")
