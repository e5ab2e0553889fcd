"""The C headers read as the one statement of the ABI: the GS_* integer constants, the structs and the gs_* prototypes of
include/graphslam.h and include/graphslam_debug.h, turned into ctypes layouts, numpy record dtypes and argtypes / restype.

Nothing is guessed: a type token the tables below do not hold, or a declaration that is neither a define, a struct nor a
prototype, raises at import with the header line.

How a declared type becomes a ctypes type (Abi.prototype):
  a scalar by value (int, int32_t, uint32_t, int64_t, double, float ...)  the matching ctypes scalar
  gs_graph * / gs_slam * / gs_shell * (an opaque handle), as a return too   c_void_p
  a handle **                                                               POINTER(c_void_p)
  any pointer parameter whose name begins with dev_                         c_void_p (callers pass DeviceArray.ptr)
  a pointer to a struct with a ctypes mirror (Abi.mirror)                   POINTER(mirror)
  a pointer to a record struct (Abi.dtype: handed over as a numpy array)    c_void_p
  any other pointer to a scalar, `const double pose[3]` included            POINTER(that scalar)
  const char * / const char *const * / void *                               c_char_p / POINTER(c_char_p) / c_void_p
  return types                                                              as declared
"""
import ctypes as C
import re

import numpy as np

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "double": C.c_double, "float": C.c_float}
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w*)\s*(\[[^\]]*\])?$")     # type, stars, name, [extent]


class HeaderError(ValueError):
    pass


class Abi:
    def __init__(self):
        self.defines = {}       # GS_NAME -> int
        self.handles = set()    # opaque structs: typedef struct gs_graph gs_graph;
        self.structs = {}       # name -> [(field, scalar type name, extent or None)]
        self.protos = {}        # name -> (origin, return (type, stars), [(type, stars, parameter name)])
        self.mirrors = {}       # struct name -> ctypes.Structure subclass
        self.records = {}       # struct name -> numpy dtype

    # ---- reading
    def read(self, text, origin="<header>"):
        """collect the defines, structs and prototypes of one header's text"""
        text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: re.sub(r"[^\n]", " ", m.group()), text, flags=re.S)   # comments out, lines kept
        def fail(pos, why):
            line = text.count("\n", 0, pos) + 1
            raise HeaderError("%s:%d: %s: %s" % (origin, line, why, " ".join(text.split("\n")[line - 1].split())))
        body, at = [], 0
        for ln in text.split("\n"):                         # preprocessor lines out; the integer GS_* defines kept
            if ln.lstrip().startswith("#"):
                m = re.match(r"\s*#\s*define\s+(GS_\w+)\s+(\S.*?)\s*$", ln)
                if m:
                    if not re.fullmatch(r"-?\d+", m.group(2)):
                        fail(at, "define of something other than an integer")
                    self.defines[m.group(1)] = int(m.group(2))
                ln = ""
            body.append(ln); at += len(ln) + 1
        text = re.sub(r'extern\s+"C"\s*\{', lambda m: " " * len(m.group()), "\n".join(body))
        depth, start = 0, 0
        for pos, ch in enumerate(text):                     # statements: up to a ';' outside braces
            if ch == "{":
                depth += 1
            elif ch == "}":
                if depth == 0:                              # the end of extern "C"
                    start = pos + 1
                depth = max(depth - 1, 0)
            elif ch == ";" and depth == 0:
                stmt = text[start:pos]; lead = len(stmt) - len(stmt.lstrip()); start = pos + 1
                if stmt.strip():
                    self._statement(" ".join(stmt.split()), origin, lambda why, p=pos - len(stmt) + lead: fail(p, why))
        if text[start:].strip():
            fail(start + len(text[start:]) - len(text[start:].lstrip()), "unfinished declaration")

    def _decl(self, s, fail):
        m = _DECL.match(s)
        if not m:
            fail("cannot read the declaration %r" % s)
        base, stars, name, extent = m.groups()
        return base, stars.count("*"), name, extent

    def _statement(self, s, origin, fail):
        m = re.fullmatch(r"typedef struct (\w+) (\w+)", s)
        if m and m.group(1) == m.group(2):
            self.handles.add(m.group(1)); return
        m = re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", s)
        if m and m.group(1) == m.group(3):
            fields = []
            for d in filter(None, (d.strip() for d in m.group(2).split(";"))):
                base, rest = d.split(None, 1)
                if base not in SCALARS:
                    fail("unknown field type %r" % base)
                for one in rest.split(","):                 # int32_t a, b[4];
                    _, stars, name, extent = self._decl(base + " " + one.strip(), fail)
                    if stars or not name:
                        fail("cannot read the field %r" % one.strip())
                    fields.append((name, base, None if extent is None else self._extent(extent[1:-1], fail)))
            self.structs[m.group(1)] = fields; return
        m = re.fullmatch(r"(.*?)\b(gs_\w+) ?\((.*)\)", s)
        if m and not s.startswith("typedef"):
            rb, rs, rn, _ = self._decl(m.group(1).strip(), fail)
            if rn:                                          # two words before the name, as in `unsigned int`
                fail("cannot read the return type %r" % m.group(1).strip())
            params = [] if m.group(3).strip() == "void" else [self._decl(p.strip(), fail) for p in m.group(3).split(",")]
            params = [(b, n + (x is not None), name) for b, n, name, x in params]
            for b, n in [(rb, rs)] + [p[:2] for p in params]:
                if b not in SCALARS and b not in ("char", "void") and not b.startswith("gs_"):
                    fail("unknown type %r" % b)
            self.protos[m.group(2)] = (origin, (rb, rs), params); return
        fail("neither a define, a struct nor a gs_* prototype")

    def _extent(self, expr, fail):
        e = re.sub(r"GS_\w+", lambda m: str(self.defines[m.group()]) if m.group() in self.defines else fail("unknown constant %s" % m.group()), expr)
        if not re.fullmatch(r"[\d\s+\-*()]+", e):
            fail("cannot read the array extent %r" % expr)
        return int(eval(e))

    # ---- layouts
    def fields(self, cname, rename=()):
        """_fields_ of the struct; rename: {header name: Python name}"""
        rename = dict(rename)
        return [(rename.get(n, n), SCALARS[t] if x is None else SCALARS[t] * x) for n, t, x in self.structs[cname]]

    def mirror(self, cname, rename=()):
        """class decorator: the ctypes.Structure that stands for the struct takes its _fields_ from the header"""
        def bind(cls):
            cls._fields_ = self.fields(cname, rename); self.mirrors[cname] = cls
            return cls
        return bind

    def structure(self, pyname, cname):
        """a ctypes.Structure of the struct under the Python name given"""
        return self.mirror(cname)(type(pyname, (C.Structure,), {"__doc__": "%s (include/graphslam.h)" % cname}))

    def dtype(self, cname):
        """the struct as a numpy record dtype (it must need no padding)"""
        d = np.dtype([(n, np.dtype(SCALARS[t])) if x is None else (n, np.dtype(SCALARS[t]), x) for n, t, x in self.structs[cname]])
        if d.itemsize != C.sizeof(type("_", (C.Structure,), {"_fields_": self.fields(cname)})):
            raise HeaderError("%s has padding: it cannot be a packed numpy record" % cname)
        self.records[cname] = d
        return d

    # ---- prototypes
    def _ctype(self, fn, base, stars, pname):
        if stars == 0 and base in SCALARS:
            return SCALARS[base]
        if base in self.handles and stars in (1, 2):
            return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
        if stars and pname.startswith("dev_"):
            return C.c_void_p
        if base == "char" and stars in (1, 2):
            return C.c_char_p if stars == 1 else C.POINTER(C.c_char_p)
        if stars == 1 and (base == "void" or base in self.records):
            return C.c_void_p
        if stars == 1 and (base in self.mirrors or base in SCALARS):
            return C.POINTER(self.mirrors[base] if base in self.mirrors else SCALARS[base])
        raise HeaderError("%s: no ctypes type for %r" % (fn, " ".join(filter(None, (base, "*" * stars, pname)))))

    def prototype(self, fn, overrides={}):
        """(restype, argtypes) of the function, with the mirrors and records declared so far; overrides: {(function, parameter): ctypes type}"""
        _, (rb, rs), params = self.protos[fn]
        return self._ctype(fn, rb, rs, ""), [overrides.get((fn, name)) or self._ctype(fn, b, n, name) for b, n, name in params]
