"""The model of include/mpecdsa_hip.h that every binding emitter reads (tools/gen_rust_bindings.py, tools/gen_python_bindings.py):
the header is the one place where the C-ABI is written, and this is the one parser of it.

The header is run through `gcc -E` (comments and include guards gone), split into top-level declarations and each declaration is
kept with its C types: `load()` returns the opaque handle types, the structs (fields in order, with array lengths), the functions
(parameter names and types, return type) and the integer `#define`s.  A base type that is neither in SCALARS nor declared by the
header stops the run: an emitter never sees a type it has no word for."""
import collections
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpecdsa_hip.h")

# C scalar -> (Rust, ctypes); `void` has no ctypes scalar: it only occurs behind a pointer or as a return type
SCALARS = {"int": ("c_int", "c_int"), "unsigned": ("c_uint", "c_uint"), "long": ("c_long", "c_long"), "char": ("c_char", "c_char"),
           "uint8_t": ("u8", "c_uint8"), "int32_t": ("i32", "c_int32"), "uint32_t": ("u32", "c_uint32"), "int64_t": ("i64", "c_int64"),
           "uint64_t": ("u64", "c_uint64"), "size_t": ("usize", "c_size_t"), "float": ("f32", "c_float"), "void": ("c_void", None)}
RUST, CTYPES = 0, 1

# base: a key of SCALARS, an opaque type or a struct; ptrs: one bool per pointer level, innermost first, True = points to const;
# array: the length of an array field, else None
Type = collections.namedtuple("Type", "base ptrs array")
Model = collections.namedtuple("Model", "opaque structs funcs constants")
# opaque [name]; structs [(name, [(field, Type)])]; funcs [(name, [(param, Type)], return Type)]; constants [(name, int)]


def preprocess():
    src = subprocess.check_output(["gcc", "-E", "-P", "-x", "c", "-D__cplusplus_off", HEADER], text=True)
    # drop everything the system headers contributed: keep from the first mpe_ symbol's typedef on
    start = src.index("typedef struct mpe_ctx mpe_ctx;")
    return src[start:]


def constants():
    """`#define MPE_X 12`, `(-1)`, and the typed form `((int)841)` / `((uint32_t)0x3153504du)`: a cast of one integer literal"""
    lit = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*"
    rule = rf"^#define\s+(MPE_\w+)\s+(?:\(?{lit}\)?|\(\(\w+\)\s*{lit}\))\s*(?:/\*.*)?$"
    found = [(m.group(1), m.group(2) or m.group(3)) for m in re.finditer(rule, open(HEADER).read(), re.M)]
    return [(name, int(v, 16 if "x" in v.lower() else 10)) for name, v in found]


def split_decls(src):
    decls, depth, cur = [], 0, []
    for ch in src:
        cur.append(ch)
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif ch == ";" and depth == 0:
            d = " ".join("".join(cur).split())
            if d != ";":
                decls.append(d[:-1].strip())
            cur = []
    return decls


def parse_type(ctype, array=None):
    """'const uint32_t *' -> Type('uint32_t', (True,), None) ; 'mpe_ctx * *' -> Type('mpe_ctx', (False, False), None)"""
    const, base, ptrs = False, None, []
    for tok in ctype.replace("*", " * ").split():
        if tok == "const":
            const = True
        elif tok == "struct":
            continue
        elif tok == "*":
            ptrs.append(const)
            const = False
        else:
            base = tok
    return Type(base, tuple(ptrs), array)


def parse_fields(body):
    """'uint32_t *z, *e; int kind; uint8_t ord[4];' -> [(name, Type)]"""
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        first, *rest = [x.strip() for x in stmt.split(",")]
        m = re.match(r"(.*?)(\**)\s*(\w+)\s*(\[\d+\])?$", first)
        base = m.group(1).strip()
        for decl in [first[len(m.group(1)):]] + rest:
            dm = re.match(r"(\**)\s*(\w+)\s*(?:\[(\d+)\])?$", decl.strip())
            fields.append((dm.group(2), parse_type(base + " " + dm.group(1), int(dm.group(3)) if dm.group(3) else None)))
    return fields


def parse(src):
    opaque, structs, funcs = [], [], []
    for d in split_decls(src):
        m = re.match(r"typedef struct (\w+) (\w+)$", d)
        if m:
            opaque.append(m.group(2))
            continue
        m = re.match(r"typedef struct (?:\w+ )?\{(.*)\} (\w+)$", d)
        if m:
            structs.append((m.group(2), parse_fields(m.group(1))))
            continue
        m = re.match(r"(.*?)(\w+) ?\((.*)\)$", d)
        if not m:
            raise SystemExit(f"abi_model: cannot parse declaration: {d[:120]}")
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        params = []
        if args and args != "void":
            for a in args.split(","):
                am = re.match(r"(.*?)(\w+)$", a.strip())
                params.append((am.group(2), parse_type(am.group(1))))
        funcs.append((name, params, parse_type(ret)))
    return opaque, structs, funcs


def load():
    opaque, structs, funcs = parse(preprocess())
    known = set(SCALARS) | set(opaque) | {name for name, _ in structs}
    for where, t in ([(f"{s}.{f}", t) for s, fields in structs for f, t in fields]
                     + [(f"{fn}({p})", t) for fn, params, _ in funcs for p, t in params] + [(f"{fn}()", ret) for fn, _, ret in funcs]):
        if t.base not in known:
            raise SystemExit(f"abi_model: {where}: no entry for the C type `{t.base}` (SCALARS of tools/abi_model.py)")
    return Model(opaque, structs, funcs, constants())


def wrap(prefix, items, suffix, indent, width=128):
    """prefix item, item, ... suffix, broken before `width` columns; continuation lines start with `indent`"""
    lines, cur = [], prefix
    for i, it in enumerate(items):
        piece = it + (", " if i + 1 < len(items) else "")
        if len(cur) + len(piece) > width and cur.strip():
            lines.append(cur.rstrip())
            cur = indent + piece
        else:
            cur += piece
    lines.append(cur + suffix)
    return "\n".join(lines)


def emit(outputs, check, tool):
    """outputs {path: text}: writes them, or with check only reports the stale ones -> the exit status of the emitter"""
    stale = [path for path, text in outputs.items() if not os.path.exists(path) or open(path).read() != text]
    if check:
        if stale:
            print(f"stale (run {tool}):", *stale)
        return 1 if stale else 0
    for path in stale:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "w").write(outputs[path])
    return 0
