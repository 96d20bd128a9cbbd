"""The argument rules of a reprojection of caller planes (polaris_amd/csrc/reproject_io.h, check_reproject), stated as ONE table of
single violations that tests/test_reproject_args_cpu.py applies to the four host entries and tests/test_gpu_reproject_entries.py to
the three device entries: a new rule adds one row.

A call is a dict of named arguments -- arrays, a TemporalParams, integers, or None for a null pointer -- which raw() hands to an
entry in the order of its C signature, with nothing checked on the way.  The frame is 8 x 4 with 2 instances and 2 triangles."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import motion_oracle as MO
import temporal_oracle as TO
import vertex_motion_oracle as VO
from polaris_amd import ctypes_api as T

F = np.float32
W, H = 8, 4
BAD_ARGUMENT = 2                               # POLARIS_E_BAD_ARGUMENT
MAX_INSTANCES, MAX_TRIANGLES = 1 << 20, 1 << 24  # temporal.h: kTpMaxInstances, kTpMaxTriangles
MAX_PIXELS = 1 << 26
DUMMY = 64                                     # a pointer nothing may read or write: the refusal comes first

# the C signatures (the device entries': the same behind the handle; there is no device entry for "reproject_moments")
ORDER = {
    "reproject": "hist pg pa pe pf g a e f W H p prior",
    "reproject_moments": "hist hvar pg pa pe pf g a e f W H p prior prior2",
    "reproject_motion": "hist pg pa pi pe pf g a i e f W H n pt ct p hvar prior prior2",
    "reproject_deform": "hist pg pa pi pe pf g a i e f W H n pt ct p hvar prior prior2 hit v pv nt",
}
ORDER = {k: v.split() for k, v in ORDER.items()}
DEVICE = {"reproject": "reproject_planes", "reproject_motion": "reproject_motion_planes", "reproject_deform": "reproject_deform_planes"}
PLANES = ("hist", "pg", "pa", "g", "a", "prior", "hvar", "prior2", "pi", "i", "hit")   # frame-sized: dummies where the frame is refused


@functools.lru_cache(maxsize=None)
def _scene() -> dict:
    """One quad of two triangles in front of the camera, the first in instance 0 (STATIC), the second in instance 1 (MOVED), both
    deformed a little between the history and now; a random history and history VARIANCE plane."""
    import test_temporal_cpu as TC
    from polaris_amd import scenes as S

    rng = np.random.default_rng(3)
    old = VO.quad_tris(-1.0, 1.0, -0.6, 0.6, -3.0)
    new = old.copy()
    new[:, 2] += (0.03 * np.sin(3.0 * old[:, 0] + old[:, 1])).astype(F)
    tri_inst, tri_leaf = np.array([0, 1]), np.full(2, T.BXDF_DIFFUSE)
    pe, pf = TO.pinhole((0, 0, 0))
    e, f = TO.pinhole((0.04, 0.02, 0))
    then, now = [np.eye(4), S.translation((0.05, 0.02, 0))], [np.eye(4), S.translation((0.1, -0.03, -0.05))]
    pg, pa, pi, _ = VO.cast(pe, pf, W, H, old, tri_inst, tri_leaf, then)
    g, a, i, hit = VO.cast(e, f, W, H, new, tri_inst, tri_leaf, now)
    return dict(hist=TC.history_planes(rng, H, W), pg=pg, pa=pa, pi=pi, pe=pe, pf=pf, g=g, a=a, i=i, e=e, f=f,
                pt=np.stack([MO.inv16(w) for w in then]), ct=np.stack([MO.inv16(w) for w in now]), hit=hit, v=new, pv=old,
                hvar=(rng.random((H, W, 4)) * 2).astype(F))


def valid(entry: str, moments: bool | None = None) -> dict:
    """A call the entry accepts (fresh copies: a row may change them).  moments: with the history's VARIANCE plane and PRIOR2 (default:
    only where the entry demands them)."""
    d = {k: np.ascontiguousarray(v, np.uint32 if k in ("pi", "i", "hit") else F).copy() for k, v in _scene().items()}
    d.update(W=W, H=H, n=2, nt=2, p=T.temporal_params(**T.TEMPORAL_DEFAULTS), prior=np.zeros((H, W, 4), F), prior2=np.zeros((H, W, 4), F))
    if not (entry == "reproject_moments" if moments is None else moments):
        d["hvar"] = d["prior2"] = None
    return {k: d[k] for k in ORDER[entry]}


def raw(fn, entry: str, d: dict, *head) -> int:
    """fn(*head, the call's arguments in the entry's order): the code it returns."""
    def c_arg(x):
        return C.byref(x) if isinstance(x, T.TemporalParams) else x.ctypes.data if isinstance(x, np.ndarray) else x
    return fn(*head, *[c_arg(d[k]) for k in ORDER[entry]])


def _params(**kw):
    def change(d):
        d["p"] = T.temporal_params(**{**T.TEMPORAL_DEFAULTS, **kw})
    return change


def _struct_size(delta):
    def change(d):
        d["p"] = T.temporal_params(**T.TEMPORAL_DEFAULTS)
        d["p"].struct_size += delta
    return change


def _frame(w, h):
    def change(d):
        d.update(W=w, H=h, **{k: DUMMY for k in PLANES if d.get(k) is not None})
    return change


def _set(**kw):
    return lambda d: d.update(kw)


POINTERS = ("hist", "pg", "pa", "pe", "pf", "g", "a", "e", "f", "p", "prior", "pi", "i", "pt", "ct", "hit", "v", "pv")
# (name, the arguments it needs -- the row applies to the entries that take them all --, the change)
VIOLATIONS = [(f"null {k}", (k,), _set(**{k: None})) for k in POINTERS] + [
    ("struct_size + 4", (), _struct_size(4)),
    ("struct_size - 4", (), _struct_size(-4)),
    ("max_history 4097", (), _params(max_history=4097)),
    ("normal_threshold above 1", (), _params(normal_threshold=np.nextafter(F(1), F(2)))),
    ("normal_threshold below -1", (), _params(normal_threshold=np.nextafter(F(-1), F(-2)))),
    ("normal_threshold NaN", (), _params(normal_threshold=float("nan"))),
    ("depth_threshold below 0", (), _params(depth_threshold=-1e-30)),
    ("depth_threshold above 1e6", (), _params(depth_threshold=np.nextafter(F(1e6), F(2e6)))),
    ("depth_threshold NaN", (), _params(depth_threshold=float("nan"))),
    ("W = 0", (), _frame(0, H)),
    ("H = 0", (), _frame(W, 0)),
    ("W * H = 2^26 + 1", (), _frame(MAX_PIXELS + 1, 1)),
    ("n_instances = 0", ("n",), _set(n=0)),
    ("n_instances = max + 1", ("n",), _set(n=MAX_INSTANCES + 1)),
    ("num_triangles = 0", ("nt",), _set(nt=0)),
    ("num_triangles = max + 1", ("nt",), _set(nt=MAX_TRIANGLES + 1)),
    ("history_variance without prior2", ("hvar",), lambda d: d.update(hvar=np.zeros((H, W, 4), F), prior2=None)),
    ("prior2 without history_variance", ("hvar",), lambda d: d.update(hvar=None, prior2=np.zeros((H, W, 4), F))),
]
# the values at the bounds, which are accepted: the rows above sit just outside them
ACCEPTED = [("max_history 4096", _params(max_history=4096)), ("max_history 0", _params(max_history=0)),
            ("normal_threshold 1", _params(normal_threshold=1.0)), ("normal_threshold -1", _params(normal_threshold=-1.0)),
            ("depth_threshold 0", _params(depth_threshold=0.0)), ("depth_threshold 1e6", _params(depth_threshold=1e6))]


def rows(entry: str):
    """[(name, change)] of the violations that apply to the entry."""
    return [(name, change) for name, needs, change in VIOLATIONS if all(k in ORDER[entry] for k in needs)]


def violated(entry: str, change, moments: bool | None = None) -> dict:
    d = valid(entry, moments)
    change(d)
    return d
