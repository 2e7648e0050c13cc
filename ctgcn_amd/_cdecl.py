"""Reader of the C declarations of include/ctgcn_hip.h: header text in, ctypes objects out.

Pure functions on text (no file access, no torch), for the small C subset the header is written in: integer `#define`s, anonymous
enums with explicit values, `typedef struct { ... } name;` of scalars and pointers, and function prototypes.  Every directive and
every statement of the text must be one of these: whatever is not raises CDeclError quoting it, because a declaration skipped in
silence would leave an entry point unbound or a descriptor field shifted.
"""
import ctypes
import re
from collections import namedtuple

SCALARS = {
    "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
    "int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "char": ctypes.c_char,
}
_POINTEE_ONLY = ("void", "uint8_t")     # never passed or stored by value; a pointer to them is an address like any other

# `/* ... */` in its unrolled form (runs of non-stars, then stars that a `/` does not follow) and `// ...`: two thirds of the header is
# comment, and a lazy `.*?` walks it four times slower
_COMMENT = re.compile(r"/(?:\*[^*]*\*+(?:[^/*][^*]*\*+)*/|/[^\n]*)")
# after the comments a `#` can only start a directive: the patterns begin with it, which lets the search skip from one to the next
_CPLUSPLUS = re.compile(r"#[ \t]*ifdef[ \t]+__cplusplus\b.*?#[ \t]*endif\b", re.S)     # the `extern "C"` bracket
_DIRECTIVE = re.compile(r"#[ \t]*(?:(?:include|ifndef|endif)\b[^\n]*|define[ \t]+(\w+)(?:[ \t]+([-+]?\w+))?[ \t]*$|([^\n]*))", re.M)
_BLOCK = re.compile(r"\s*(typedef\s+struct|enum)\s*\{([^{}]*)\}\s*(\w*)\s*")
_ENUMERATOR = re.compile(r"\s*(\w+)\s*=\s*([-+]?\w+)\s*")
_PROTOTYPE = re.compile(r"\s*([^()]*?)(\w+)\s*\(([^()]*)\)\s*")
_BASE = re.compile(r"\s*(?:const\s+)?\w+")
_DECL = re.compile(r"\s*(const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(\w*)\s*")       # [const] base [*[const]]... [name]

Header = namedtuple("Header", "functions structs constants")


class CDeclError(ValueError):
    pass


def _fail(why, decl):
    raise CDeclError("%s: `%s`" % (why, " ".join(decl.split())))


def _int(literal, decl):
    try:
        return int(literal, 0)
    except (TypeError, ValueError):
        _fail("not an integer constant", decl)


def _ctype(decl, structs, param):
    """(name, ctypes type) of one declaration; the type is None for a bare `void`."""
    m = _DECL.fullmatch(decl)
    if not m:
        _fail("unreadable declaration (arrays, function pointers and bit-fields are not supported)", decl)
    const, typ, stars, name = m.groups()
    scalar = SCALARS.get(typ)
    if scalar is None and typ not in _POINTEE_ONLY and typ not in structs:
        _fail("unknown base type `%s`" % typ, decl)
    if not stars:
        if scalar is None and (typ != "void" or name):
            _fail("`%s` by value" % typ, decl)
        return name, scalar
    if param and scalar is not None and stars.strip() == "*":
        if typ == "char":
            return name, ctypes.c_char_p
        if not const and name.endswith("_host"):
            return name, ctypes.POINTER(scalar)
    return name, ctypes.c_void_p


def parse(text):
    """Header(functions {name: (restype, [argtypes])}, structs {typedef name: [(field, ctype), ...]}, constants {name: int})."""
    functions, structs, constants = {}, {}, {}

    def directive(m):
        name, value, other = m.groups()
        if other is not None:
            _fail("directive is neither an include guard nor `#define NAME <integer>`", m.group())
        if value:       # a bare `#define NAME` is the include guard
            constants[name] = _int(value, m.group())
        return " "

    code = _DIRECTIVE.sub(directive, _CPLUSPLUS.sub(" ", _COMMENT.sub(" ", text)))
    *pieces, rest = code.split(";")
    stmt = ""
    for piece in pieces:        # a statement: up to the first `;` outside braces
        stmt += piece
        if stmt.count("{") > stmt.count("}"):
            stmt += ";"
            continue
        block, proto = _BLOCK.fullmatch(stmt), _PROTOTYPE.fullmatch(stmt)
        if block and block.group(1) == "enum" and not block.group(3):
            for item in filter(str.strip, block.group(2).split(",")):
                m = _ENUMERATOR.fullmatch(item)
                if not m:
                    _fail("enumerator without an explicit integer value", item)
                constants[m.group(1)] = _int(m.group(2), item)
        elif block and block.group(1) != "enum" and block.group(3):
            fields = structs[block.group(3)] = []
            for member in filter(str.strip, block.group(2).split(";")):
                base = _BASE.match(member)      # `const int32_t *a, *b`: the declarators share the base type
                if not base:
                    _fail("unreadable struct member", member)
                for d in member[base.end():].split(","):
                    field, typ = _ctype(base.group() + " " + d, structs, False)
                    if not field or typ is None:
                        _fail("struct member without a name", member)
                    fields.append((field, typ))
        elif proto and proto.group(3).strip() and proto.group(2) not in functions:
            args = [_ctype(p, structs, True)[1] for p in proto.group(3).split(",")]
            if args == [None]:      # (void)
                args = []
            if None in args:
                _fail("void parameter", stmt)
            functions[proto.group(2)] = (_ctype(proto.group(1), structs, True)[1], args)
        elif stmt.strip():
            _fail("neither an anonymous enum, a `typedef struct { ... } name`, nor a function prototype declared once", stmt)
        stmt = ""
    if (stmt + rest).strip():
        _fail("statement without its `;`, or unbalanced braces", stmt + rest)
    return Header(functions, structs, constants)


def functions(text):
    return parse(text).functions


def structs(text):
    return parse(text).structs


def constants(text):
    return parse(text).constants
