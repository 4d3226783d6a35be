"""The ctypes binding of liblush_march.so, read from its contract include/lush_march.h: signatures, structs and constants are
stated there and nowhere else ("One source for the ABI").

Three patterns cover the header as it is written: `#define LUSH_X <integer>`, `typedef struct [tag] { ... } name;` and
`ret lush_name(args);`.  A declaration that fits none of them, or uses a type that is not in the table below, raises:
the reader never guesses (a wrong guess is a float passed where the library expects a device pointer).
"""
import ctypes as C
import re
from types import SimpleNamespace

_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t, "lush_stream_t": C.c_void_p}
_INT = r"0[xX][0-9a-fA-F]+|0|[1-9][0-9]*"
_DECL = r"(\*?)\s*(\w+)\s*(?:\[(\d+)\])?"      # [*] name [N]


def parse(text: str, header: str = "lush_march.h") -> SimpleNamespace:
    """consts {LUSH_X: int}, structs {header name: ctypes.Structure class}, protos {lush_name: (argtypes, restype)}.
    `header` names the file being read, for the error messages."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, structs, protos, classes = {}, {}, {}, {}

    def ctype(base, star, where):
        # a pointer to a struct of this header is typed; every other pointer (device data, host out-parameters) is a void*,
        # which takes None, integers, byref(...) and ctypes arrays
        base = " ".join(re.sub(r"\bconst\b", " ", base).split())
        if star:
            return C.POINTER(structs[base]) if base in structs else C.c_void_p
        if base not in _SCALARS:
            raise ValueError(f"{header}: unknown type `{base}` in `{where}`")
        return _SCALARS[base]

    for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(LUSH_\w+)(.*)$", text, flags=re.M):
        if body.strip():      # (an empty body is the include guard)
            if not re.fullmatch(_INT, body.strip()):
                raise ValueError(f"{header}: `#define {name}{body}` is not an integer constant")
            consts[name] = int(body.strip(), 0)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', "", text)
    if n_extern:
        text = text.rstrip().removesuffix("}")

    def struct(m):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            first, *more = decl.split(",")
            head = re.fullmatch(r"(\w[\w\s]*?)\s*" + _DECL, first.strip())
            rest = [re.fullmatch(_DECL, d.strip()) for d in more]
            if not head or not all(rest):
                raise ValueError(f"{header}: cannot read the field `{decl}` of {m.group(2)}")
            for star, field, count in [head.groups()[1:]] + [r.groups() for r in rest]:
                t = ctype(head.group(1), star, f"{decl}` of `{m.group(2)}")
                fields.append((field, t * int(count) if count else t))
        # structs that differ in `const` alone (lush_mlp_grads / lush_mlp_params) are ONE class: byref() of it serves both
        key = tuple(fields)
        if key not in classes:
            classes[key] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        structs[m.group(2)] = classes[key]
        return ""
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)

    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        if stmt == "typedef void* lush_stream_t":
            continue
        m = re.fullmatch(r"(\w[\w\s]*?\s*\*?)\s*\b(lush_\w+)\s*\((.*)\)", stmt)
        if not m:
            raise ValueError(f"{header}: cannot read the declaration `{stmt}`")
        ret, name, args = m.groups()
        argtypes = []
        for arg in ([] if args.strip() == "void" else args.split(",")):
            a = re.fullmatch(r"(\w[\w\s]*?)\s*(\*?)\s*(\w+)", arg.strip())
            if not a:
                raise ValueError(f"{header}: cannot read the parameter `{arg.strip()}` of `{stmt}`")
            argtypes.append(ctype(a.group(1), a.group(2), stmt))
        is_str = re.sub(r"\s", "", ret) == "constchar*"
        protos[name] = (argtypes, C.c_char_p if is_str else ctype(ret, "", stmt))
    return SimpleNamespace(consts=consts, structs=structs, protos=protos)
