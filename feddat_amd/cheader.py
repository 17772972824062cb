"""Reader of the C ABI headers (include/feddat_hip.h and its extension headers include/feddat_hip_prompt.h and
include/feddat_hip_albef.h): what feddat_amd/lib.py binds with ctypes.

Not a C parser: it reads the constructs these headers contain -- block comments, preprocessor lines, `typedef struct`
(complete or opaque), int / long functions named feddat_* -- and raises HeaderError on anything else, at import: a type it
does not know, a declaration it cannot read or any text left over stops the binding instead of being bound by a guess.
Pure Python (no torch, nothing from the package), so it is tested without the library.

MAIN / PROMPT / ALBEF, one Header per file:
  functions  name -> (restype, [(ctype, parameter name), ...])                in declaration order
  structs    typedef name -> [(field name, ctype), ...]                       scalars, pointers and fixed arrays
  types      typedef name -> the ctypes.Structure class with those _fields_
  defines    X of every `#define FEDDAT_X <number>` -> int | float
"""
import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "unsigned": C.c_uint, "uint32_t": C.c_uint,
           "hipStream_t": C.c_void_p}
POINTEES = {"void", "char", "unsigned char", "uint8_t", "int64_t", "int", "long", "float"}     # + the header's own typedefs
DECLARATION = r"^(?:int|long) (feddat_[a-z0-9_]+)\("     # a line that looks like an entry point (tests/test_cabi_cpu.py)
_BASE = re.compile(r"(?:const\s+)?(unsigned char|\w+)\s*(.*)", re.S)
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\s*)?)*)(\w+)(?:\[(\d+)\])?")


class HeaderError(ValueError):
    pass


class Header:
    def __init__(self, filename, base=None):
        self.functions, self.structs, self.defines = {}, {}, {}
        self.types = dict(base.types) if base else {}            # an extension header sees the structs of the one it includes
        self._opaque = set(base._opaque) if base else set()
        self.path = os.path.join(INCLUDE, filename)
        with open(self.path) as f:
            raw = f.read()
        text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
        text = re.sub(r"^#define FEDDAT_(\w+)[ \t]+(\S.*)$", self._define, text, flags=re.M)
        text = re.sub(r"^#.*$|^typedef struct ihipStream_t\* hipStream_t;$|^extern \"C\" \{$|^\}$", "", text, flags=re.M)
        text = re.sub(r"typedef struct (\w+) \1;", lambda m: self._opaque.add(m.group(1)) or "", text)
        text = re.sub(r"typedef struct\s*\w*\s*\{(.*?)\}\s*(\w+);", self._struct, text, flags=re.S)
        text = re.sub(r"^(int|long) (feddat_[a-z0-9_]+)\(([^()]*)\);", self._function, text, flags=re.M)
        if text.strip():
            raise HeaderError(f"{self.path}: cannot read {text.strip()[:200]!r}")
        if len(self.functions) != len(re.findall(DECLARATION, raw, flags=re.M)):
            raise HeaderError(f"{self.path}: {len(self.functions)} functions parsed, another number of lines look like one")

    def _define(self, m):
        v = re.fullmatch(r"\(?(-?\d+|-?\d*\.\d+(?:e-?\d+)?f?)\)?", m.group(2).strip())
        if not v:
            raise HeaderError(f"{self.path}: FEDDAT_{m.group(1)} is no number: {m.group(2)!r}")
        self.defines[m.group(1)] = int(v.group(1)) if v.group(1).lstrip("-").isdigit() else float(v.group(1).rstrip("f"))
        return ""

    def _declare(self, text):
        """`const float* A`, `long sa_i, sa_k`, `const void *wd[2]`, `float* const* grads_dev` -> [(name, ctype), ...]"""
        head = _BASE.fullmatch(text.strip())
        base, rest = head.groups() if head else ("", "")
        out = []
        for d in rest.split(","):
            m = _DECLARATOR.fullmatch(d.strip())
            if not m:
                raise HeaderError(f"{self.path}: cannot read the declaration {text.strip()!r}")
            stars, name, count = m.group(1).count("*"), m.group(2), m.group(3)
            if stars == 0 and base in SCALARS:
                t = SCALARS[base]
            elif stars == 1 and base in self.types and not name.endswith("_dev"):       # _dev: a device-resident table
                t = C.POINTER(self.types[base])
            elif stars and (base in POINTEES or base in self.types or base in self._opaque):
                t = C.c_void_p
            else:
                raise HeaderError(f"{self.path}: unknown type in {text.strip()!r}")
            out.append((name, t * int(count) if count else t))
        return out

    def _struct(self, m):
        fields = [f for stmt in m.group(1).split(";") if stmt.strip() for f in self._declare(stmt)]
        self.structs[m.group(2)] = fields
        self.types[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return ""

    def _function(self, m):
        if m.group(2) in self.functions:
            raise HeaderError(f"{self.path}: {m.group(2)} is declared twice")
        params = [] if m.group(3).strip() == "void" else [self._declare(p)[0] for p in m.group(3).split(",")]
        self.functions[m.group(2)] = (SCALARS[m.group(1)], [(t, name) for name, t in params])
        return ""


MAIN = Header("feddat_hip.h")
PROMPT = Header("feddat_hip_prompt.h", MAIN)
ALBEF = Header("feddat_hip_albef.h", MAIN)
