"""include/dalle_hip.h read as data: the ctypes signature of every dmi_* function, the fields of its structs and the values of
its DMI_* constants.  The header is the one description of the C ABI; nothing on the Python side repeats it.

Standard library only, and neither torch nor the library is needed: parse() takes the header's text, header() reads the
tree's own header once per process, declare(L) types any ctypes.CDLL of the library (a build loaded by path included)."""
import collections
import ctypes
import functools
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include", "dalle_hip.h")

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
FUNCTION = re.compile(r"([^;{}()]*?)\b(dmi_\w+)\s*\(([^()]*)\)\s*;")
STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")
ENUM = re.compile(r"typedef\s+enum\s*\{([^{}]*)\}\s*dmi_status\s*;")
DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(DMI_\w+)[ \t]+(\S+)[ \t]*$", re.M)

Header = collections.namedtuple("Header", "functions structs constants")
"""functions: name -> (restype, [argtypes], [parameter names]); structs: name -> [(field, ctype)]; constants: name -> int"""


class HeaderError(ValueError):
    pass


def ctype(decl, where):
    """the one type rule: scalars by name, const char* -> c_char_p, every other pointer -> c_void_p"""
    words = " ".join(decl.replace("*", " * ").split())
    if words == "const char *":
        return ctypes.c_char_p
    if "*" in words:
        return ctypes.c_void_p
    if words not in SCALARS:
        raise HeaderError(f"{where}: unknown type {words!r}")
    return SCALARS[words]


def _members(text, sep, owner):
    """[(name, ctype)] of a parameter list or a struct body: every item is a type followed by the member's name"""
    out = []
    for item in (i.strip() for i in text.split(sep)):
        if item and item != "void":
            m = re.fullmatch(r"(.*?)(\w+)", item, re.S)
            if not m:
                raise HeaderError(f"{owner}: cannot read {item!r}")
            out.append((m.group(2), ctype(m.group(1), f"{owner}, {m.group(2)}")))
    return out


def parse(text):
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {name: int(value, 0) for name, value in DEFINE.findall(text)}
    for body in ENUM.findall(text):
        constants.update((name, int(value, 0)) for name, value in re.findall(r"(\w+)\s*=\s*(-?\w+)", body))
    structs = {name: _members(body, ";", name) for name, body in STRUCT.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", STRUCT.sub("", ENUM.sub("", text)), flags=re.M)
    functions = {}
    for res, name, params in FUNCTION.findall(text):
        members = _members(params, ",", name)
        functions[name] = (ctype(res, f"{name}, return value"), [t for _, t in members], [n for n, _ in members])
    left = re.search(r"\bdmi_\w+\s*\(", FUNCTION.sub("", text))
    if left:
        raise HeaderError(f"{left.group(0)}...: not a declaration this reader understands")
    return Header(functions, structs, constants)


@functools.lru_cache(maxsize=None)
def header():
    """the parse of the tree's include/dalle_hip.h, read once per process"""
    with open(HEADER_PATH) as f:
        return parse(f.read())


def declare(L):
    """sets restype and argtypes of every declared function on the ctypes library L"""
    for name, (res, args, _) in header().functions.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
