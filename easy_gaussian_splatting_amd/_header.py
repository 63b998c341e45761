"""Reads the C ABI out of include/gs_raster.h: the ctypes signature and the parameter names of every `gs_*` prototype and the
value of every integer `#define`.  Strict: it knows the few forms the header uses and raises `HeaderError` on anything else, so
that a new form is met at import and not as a misaligned argument list in a kernel launch."""
from __future__ import annotations

import ast
import ctypes as ct
import operator
import re

_BY_VALUE = {"int": ct.c_int, "int64_t": ct.c_int64, "size_t": ct.c_size_t, "float": ct.c_float, "double": ct.c_double,
             "int32_t": ct.c_int32, "uint32_t": ct.c_uint32, "uint64_t": ct.c_uint64}
_RETURNS = {**_BY_VALUE, "const char*": ct.c_char_p, "void": None}
_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.USub: operator.neg, ast.UAdd: operator.pos}


class HeaderError(ValueError):
    pass


def _int_expr(node, env):
    """Integer literals, earlier defines, + - * and parentheses; anything else raises."""
    if isinstance(node, ast.Constant) and type(node.value) is int:
        return node.value
    if isinstance(node, ast.Name):
        return env[node.id]
    if isinstance(node, (ast.UnaryOp, ast.BinOp)) and type(node.op) in _OPS:
        operands = [node.operand] if isinstance(node, ast.UnaryOp) else [node.left, node.right]
        return _OPS[type(node.op)](*(_int_expr(n, env) for n in operands))
    raise TypeError(type(node).__name__)


def _define(line, defines):
    m = re.fullmatch(r"#\s*define\s+(\w+)(?![\w(])(.*)", line, re.S)   # (not a function-like macro)
    if not m:
        raise HeaderError(f"cannot read the preprocessor line `{line}`")
    name, body = m.group(1), m.group(2).strip()
    if body:   # (none: the include guard, a switch)
        try:
            defines[name] = _int_expr(ast.parse(body, mode="eval").body, defines)
        except (SyntaxError, KeyError, TypeError) as e:
            raise HeaderError(f"#define {name}: `{body}` is not an integer expression over earlier defines ({e!r})") from None


def _parameter(text, func):
    m = re.fullmatch(r"(.*?)([A-Za-z_]\w*)\s*(\[\s*\w*\s*\])?", text, re.S)   # type, name, [n]
    ctype = " ".join(w for w in m.group(1).split() if w != "const") if m else None
    if m and ("*" in ctype or m.group(3)):
        return m.group(2), ct.c_void_p
    if ctype not in _BY_VALUE:
        raise HeaderError(f"{func}: cannot map the parameter `{text}` to a ctypes type")
    return m.group(2), _BY_VALUE[ctype]


def parse(text):
    """(signatures: name -> (restype, [argtypes]), params: name -> [parameter names], defines: name -> int), in the header's order."""
    # comments away, their line breaks kept: a preprocessor line stays a line
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S).replace("\\\n", " ")
    signatures, params, defines, code = {}, {}, {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
        elif not re.match(r"#\s*(include|ifdef|ifndef|endif)\b", line.strip()):   # (#ifndef X / #define X: the header's own value)
            _define(line.strip(), defines)
    for decl in re.sub(r'extern\s+"C"\s*\{', " ", "\n".join(code)).split(";"):
        decl = decl.strip().lstrip("}").strip()   # (the brace that closes extern "C")
        if not decl:
            continue
        m = re.fullmatch(r"(.+?)\b(gs_\w+)\s*\((.*)\)", decl, re.S)
        if not m:
            name = re.search(r"\bgs_\w+", decl)
            raise HeaderError(f"cannot read the declaration of {name.group() if name else '`' + ' '.join(decl.split()) + '`'}")
        ret, name, plist = " ".join(m.group(1).split()).replace(" *", "*"), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise HeaderError(f"{name}: cannot map the return type `{ret}` to a ctypes type")
        if name in signatures:
            raise HeaderError(f"{name} is declared twice")
        pairs = [] if plist in ("", "void") else [_parameter(p.strip(), name) for p in plist.split(",")]
        signatures[name], params[name] = (_RETURNS[ret], [t for _, t in pairs]), [n for n, _ in pairs]
    return signatures, params, defines
