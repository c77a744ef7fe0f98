"""The one reader of include/gsplat_mi355.h for the suite, and the one place that builds the library when it is missing.

parse() turns the header into its integer constants, its structs (every field's name, C type and array length) and its
function declarations (return type and every parameter's C type).  The C subset is the header's own: the fixed-width
integers, size_t, int, float, double, char, void, the Gs* structs, const, pointers, pointers to pointers and several
declarators per declaration (`int32_t W, H;`).  Anything else is an AbiHeaderError, never skipped: what parse() returns
is all the header declares.  tests/test_cabi_host.py holds gsplat_mi355/_lib.py against it."""
import collections
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3dgs-avatar-release_amd")
SCALARS = ("int32_t", "int64_t", "uint8_t", "uint32_t", "uint64_t", "size_t", "int", "float", "double", "char")

# `const float*` = ("float", True, 1); `float* const*` = ("float", False, 2): `const` is the pointee's (the scalar's own
# at depth 0), a const between the stars changes nothing about the ABI and is dropped
CType = collections.namedtuple("CType", "base const depth")
Field = collections.namedtuple("Field", "name type length")  # length: None, or the elements of an array field
Function = collections.namedtuple("Function", "name restype params")  # params: [(name, CType)]
Header = collections.namedtuple("Header", "constants structs functions")  # dicts in the header's order


class AbiHeaderError(ValueError):
    pass


_build = None


def build_module():
    """3dgs-avatar-release_amd/build.py as a module (SOURCES, STRICT, hipcc(), build())."""
    global _build
    if _build is None:
        spec = importlib.util.spec_from_file_location("gsplat_build", os.path.join(PKG, "build.py"))
        _build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_build)
    return _build


def lib():
    """gsplat_mi355._lib, with the shared library built first if it is not there."""
    from gsplat_mi355 import _lib
    if not os.path.exists(_lib.LIB_PATH):
        build_module().build()
    return _lib


def text():
    """The header as it is written, comments included (the capture-safe lists live in a comment)."""
    with open(os.path.join(ROOT, "include", "gsplat_mi355.h")) as f:
        return f.read()


_SPEC = r"((?:const\s+)?\w+(?:\s+const\b)?)"      # `const float`, `int32_t`, `float const`
_STARS = r"((?:\*\s*(?:const\b\s*)?)*)"           # ``, `*`, `**`, `* const*`
_INT = re.compile(r"^\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*\)?$")


def _int(s, what):
    m = _INT.match(s.strip())
    if not m:
        raise AbiHeaderError("%s: not an integer: %r" % (what, s))
    return int(m.group(1), 0)


def _ctype(spec, stars, known, what):
    words = spec.split()
    base = [w for w in words if w != "const"]
    if len(base) != 1 or base[0] not in known:
        raise AbiHeaderError("%s: unknown type %r" % (what, spec))
    return CType(base[0], "const" in words, stars.count("*"))


def _preprocess(src):
    """(the C text of the header with every directive taken out, {name: value} of its #defines)."""
    if '"' in re.sub(r'extern\s+"C"', "", src):
        raise AbiHeaderError("a string literal outside extern \"C\"")
    defines, kept, stack = collections.OrderedDict(), [], []
    for line in src.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            if not any(skip for skip in stack):
                kept.append(line)
            continue
        if s.endswith("\\"):
            raise AbiHeaderError("a continued directive: %r" % s)
        m = re.match(r"^#\s*(\w+)\s*(.*)$", s)
        word, rest = m.group(1), m.group(2).strip()
        if word == "ifdef" and rest == "__cplusplus":
            stack.append(True)   # the C view of the header: extern "C" and its brace are not read
        elif word == "ifndef" and re.match(r"^\w+_H$", rest):
            stack.append(False)  # the include guard
        elif word == "endif" and stack:
            stack.pop()
        elif word == "include" and not any(stack):
            pass
        elif word == "define" and not any(stack):
            m = re.match(r"^(\w+)\s*(.*)$", rest)
            name, value = m.group(1), m.group(2)
            if name in defines:
                raise AbiHeaderError("#define %s twice" % name)
            if value == "" and name.endswith("_H"):
                continue         # the include guard's own define
            defines[name] = _int(value, "#define " + name)
        else:
            raise AbiHeaderError("a directive this reader does not know: %r" % s)
    if stack:
        raise AbiHeaderError("an unclosed conditional")
    return "\n".join(kept), defines


def _fields(body, known, constants, struct):
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"^%s\s*(.*)$" % _SPEC, decl, flags=re.S)
        if not m:
            raise AbiHeaderError("%s: cannot read %r" % (struct, decl))
        for d in m.group(2).split(","):
            dm = re.match(r"^\s*%s\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*$" % _STARS, d)
            if not dm:
                raise AbiHeaderError("%s: cannot read the declarator %r of %r" % (struct, d, decl))
            stars, name, length = dm.groups()
            what = "%s.%s" % (struct, name)
            if length is not None:
                length = constants[length] if length in constants else _int(length, what)
            t = _ctype(m.group(1), stars, known, what)
            if t.depth == 0 and t.base == "void":
                raise AbiHeaderError("%s: a void field" % what)
            out.append(Field(name, t, length))
    if len({f.name for f in out}) != len(out):
        raise AbiHeaderError("%s: a field name twice" % struct)
    return out


def _params(body, known, fn):
    if body.strip() == "void":
        return []
    out = []
    for p in body.split(","):
        m = re.match(r"^\s*%s\s*%s\s*(\w+)\s*$" % (_SPEC, _STARS), p, flags=re.S)
        if not m:
            raise AbiHeaderError("%s: cannot read the parameter %r" % (fn, p))
        t = _ctype(m.group(1), m.group(2), known, "%s(%s)" % (fn, m.group(3)))
        if t.depth == 0 and t.base == "void":
            raise AbiHeaderError("%s: a void parameter" % fn)
        out.append((m.group(3), t))
    return out


_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_ENUM = re.compile(r"enum\s*(\w*)\s*\{([^{}]*)\}\s*;")
_FUNCTION = re.compile(r"%s\s*%s\s*(\w+)\s*\(([^(){};]*)\)\s*;" % (_SPEC, _STARS))


def parse(src=None):
    """Header(constants, structs, functions) of the header text `src` (default: include/gsplat_mi355.h)."""
    src = text() if src is None else src
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    if "/*" in src or "*/" in src:
        raise AbiHeaderError("an unbalanced comment")
    code, constants = _preprocess(src)
    structs, functions = collections.OrderedDict(), collections.OrderedDict()
    known = set(SCALARS) | {"void"}
    pos = 0
    while True:
        pos += len(code[pos:]) - len(code[pos:].lstrip())
        if pos == len(code):
            break
        m = _STRUCT.match(code, pos)
        if m:
            tag, body, name = m.groups()
            if tag != name or name in known:
                raise AbiHeaderError("typedef struct %s ... %s" % (tag, name))
            structs[name] = _fields(body, known, constants, name)
            known.add(name)
            pos = m.end()
            continue
        m = _ENUM.match(code, pos)
        if m:
            for item in m.group(2).split(","):
                if not item.strip():
                    continue  # (a trailing comma)
                em = re.match(r"^\s*(\w+)\s*=\s*(.+?)\s*$", item, flags=re.S)
                if not em or em.group(1) in constants:
                    raise AbiHeaderError("enum %s: cannot read %r" % (m.group(1), item))
                constants[em.group(1)] = _int(em.group(2), em.group(1))
            pos = m.end()
            continue
        m = _FUNCTION.match(code, pos)
        if m:
            spec, stars, name, body = m.groups()
            if name in functions:
                raise AbiHeaderError("%s declared twice" % name)
            functions[name] = Function(name, _ctype(spec, stars, known, name), _params(body, known, name))
            pos = m.end()
            continue
        raise AbiHeaderError("cannot read the declaration at %r" % code[pos:pos + 120])
    return Header(constants, structs, functions)
