"""ctypes mirrors of the POD structs in include/hrgym.h and include/hrgym_state.h, and the prototypes of the functions hrgym.h declares.

The mirrors are generated from the headers themselves (one source of truth); `sizeof` is cross-checked
against the compiled library (`hrg_state_bytes`) when it is loaded.
"""
import ctypes
import os
import re

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_INCLUDE = os.path.join(_ROOT, "include")

_CTYPES = {
    "double": ctypes.c_double,
    "float": ctypes.c_float,
    "int32_t": ctypes.c_int32,
    "uint32_t": ctypes.c_uint32,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "uint8_t": ctypes.c_uint8,
    "const double*": ctypes.POINTER(ctypes.c_double),
    "const float*": ctypes.c_void_p,     # host arrays of hrg_dataset_desc: handed over as addresses (numpy .ctypes.data)
    "const int64_t*": ctypes.c_void_p,
    "const void*": ctypes.c_void_p,
}


def _strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _parse(paths):
    consts, structs = {}, {}
    for path in paths:
        src = _strip_comments(open(path).read())
        for m in re.finditer(r"#define\s+(HRG_\w+)\s+(.+)", src):
            expr = m.group(2).strip()
            try:
                consts[m.group(1)] = int(eval(expr, {}, consts))
            except Exception:
                pass
        for m in re.finditer(r"enum\s*\{(.*?)\}", src, flags=re.S):
            val = -1
            for item in m.group(1).split(","):
                item = item.strip()
                if not item:
                    continue
                if "=" in item:
                    name, v = [x.strip() for x in item.split("=")]
                    val = int(eval(v, {}, consts))
                else:
                    name, val = item, val + 1
                consts[name] = val
        for m in re.finditer(r"typedef struct (\w+) \{(.*?)\}\s*(\w+);", src, flags=re.S):
            fields = []
            for decl in m.group(2).split(";"):
                decl = " ".join(decl.split())
                if not decl:
                    continue
                mm = re.match(r"(const \w+\*|\w+)\s+(.*)", decl)
                tname, rest = mm.group(1), mm.group(2)
                base = structs[tname] if tname in structs else _CTYPES[tname]
                for var in rest.split(","):
                    var = var.strip()
                    name = re.match(r"\w+", var).group(0)
                    dims = [int(eval(d, {}, consts)) for d in re.findall(r"\[([^\]]+)\]", var)]
                    t = base
                    for d in reversed(dims):
                        t = t * d
                    fields.append((name, t))
            structs[m.group(3)] = type(m.group(3), (ctypes.Structure,), {"_fields_": fields})
    return consts, structs


_SCALARS = dict({k: v for k, v in _CTYPES.items() if "*" not in k}, int=ctypes.c_int, size_t=ctypes.c_size_t)
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "void": None}


def parse_prototypes(src):
    """{name: (restype, [argtypes])} of every `hrg_*(...)` declaration in the header text `src`.  Every pointer (structs and `hrg_batch**` included) is a
    c_void_p: callers pass addresses, byref(...) or None.  A return or parameter type without a ctypes counterpart raises, naming the declaration."""
    protos, src = {}, _strip_comments(src)
    for m in re.finditer(r"([^;{}#]*?)\b(hrg_\w+)\s*\(([^()]*)\)\s*;", src):
        decl = " ".join(m.group(0).split())
        norm = lambda t: re.sub(r"\s*\*\s*", "* ", " ".join(t.split())).strip()   # noqa: E731
        ret, params = norm(m.group(1)), [norm(p) for p in m.group(3).split(",")]
        if ret not in _RETURNS:
            raise ValueError(f"include/hrgym.h: return type {ret!r} has no ctypes counterpart: {decl}")
        args = []
        for p in ([] if params == ["void"] else params):
            words = [w for w in p.split() if w != "const"]
            scalar = " ".join(words[:-1] if len(words) > 1 else words)   # (without the parameter's name)
            pointer = "*" in p or "[" in p   # (an array parameter is a pointer)
            if not pointer and scalar not in _SCALARS:
                raise ValueError(f"include/hrgym.h: parameter {p!r} has no ctypes counterpart: {decl}")
            args.append(ctypes.c_void_p if pointer else _SCALARS[scalar])
        protos[m.group(2)] = (_RETURNS[ret], args)
    skipped = sorted(set(re.findall(r"\b(hrg_\w+)\s*\(", src)) - set(protos))   # e.g. a function-pointer parameter: nested parentheses
    if skipped:
        raise ValueError(f"include/hrgym.h: cannot parse the declaration of {skipped}")
    return protos


CONST, _STRUCTS = _parse([os.path.join(_INCLUDE, "hrgym.h"), os.path.join(_INCLUDE, "hrgym_state.h")])
ModelDesc = _STRUCTS["hrg_model_desc"]
ClipTable = _STRUCTS["hrg_clip_table"]
LTT = _STRUCTS["hrg_ltt"]
Path = _STRUCTS["hrg_path"]
EnvState = _STRUCTS["hrg_env_state"]
BoxState = _STRUCTS["hrg_box_state"]
StackState = _STRUCTS["hrg_stack_state"]
HammerState = _STRUCTS["hrg_hammer_state"]
ExpertDesc = _STRUCTS["hrg_expert_desc"]
DatasetDesc = _STRUCTS["hrg_dataset_desc"]
HerDesc = _STRUCTS["hrg_her_desc"]
RolloutDesc = _STRUCTS["hrg_rollout_desc"]
ReplayDesc = _STRUCTS["hrg_replay_desc"]
SacDesc = _STRUCTS["hrg_sac_desc"]
PpoDesc = _STRUCTS["hrg_ppo_desc"]
SacHyper = _STRUCTS["hrg_sac_hyper"]
PpoHyper = _STRUCTS["hrg_ppo_hyper"]
BcDesc = _STRUCTS["hrg_bc_desc"]
DaggerDesc = _STRUCTS["hrg_dagger_desc"]
DiscDesc = _STRUCTS["hrg_disc_desc"]
EvalDesc = _STRUCTS["hrg_eval_desc"]
PROTOTYPES = parse_prototypes(open(os.path.join(_INCLUDE, "hrgym.h")).read())


def struct_to_dict(s):
    """Recursively convert a ctypes struct/array to python lists/dicts (for parity comparisons)."""
    if isinstance(s, ctypes.Structure):
        return {n: struct_to_dict(getattr(s, n)) for n, _ in s._fields_}
    if isinstance(s, ctypes.Array):
        return [struct_to_dict(x) for x in s]
    return s
