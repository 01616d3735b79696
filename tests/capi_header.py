"""The tests' own reader of ``include/planedepth_hip.h``: what the header declares, found with a few regular expressions, to hold
``planedepth_amd._capi`` (which derives its table from the same file with its own parser) and the built library against.  It
shares no code with the package."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "planedepth_hip.h")

RETURNS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_KIND_OF = {ctypes.c_void_p: "P", ctypes.c_float: "F", ctypes.c_int: "I", ctypes.c_double: "D", ctypes.c_int64: "L"}


def text():
    with open(HEADER) as f:
        return f.read()


def code():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", text(), flags=re.S)


def symbols():
    return sorted(set(re.findall(r"\b(pd_[a-z0-9_]+)\s*\(", code())))


def prototype(name):
    """(return type, [parameter, ...]) of ``name`` as the header spells them, white space normalised."""
    m = re.search(r"(\w[\w\s*]*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, code())
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return " ".join(m.group(1).split()), [] if params == ["void"] else params


def params(name):
    return prototype(name)[1]


def kinds(name):
    """One letter per parameter: P(ointer or stream), F(loat), D(ouble), L (int64_t), I (everything else: the ints)."""
    return ["P" if "*" in p or "pd_stream_t" in p else "F" if p.startswith("float") else "D" if p.startswith("double")
            else "L" if p.startswith("int64_t") else "I" for p in params(name)]


def ctypes_kinds(argtypes):
    """The same letters for a ctypes argument list (a POINTER(struct) is a P)."""
    return ["P" if issubclass(a, ctypes._Pointer) else _KIND_OF[a] for a in argtypes]


def constants():
    """{name: value} of every ``PD_X = n`` the header's enums hold."""
    return {k: int(v) for k, v in re.findall(r"\b(PD_[A-Z0-9_]+)\s*=\s*(-?\d+)", code())}


def constant(name):
    return constants()[name]


def enum(name):
    body = re.search(r"enum\s+%s\s*\{([^}]*)\}" % name, code()).group(1)
    return {k: int(v) for k, v in re.findall(r"(PD_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)}


def struct_members(name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (name, name), code()).group(1)
    return [m for decl in body.split(";") for m in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
