"""The argument contract of the batched C ABI (include/rigidbody_batch.h), pinned on the raw
entry points through ffi.lib(): which status each bad call returns, in which order the checks
run, and the messages callers match.  Every call here is refused (or has nothing to do) before
the device is touched, so the file needs no GPU.

The entry points are enumerated from the header (test_boundary.declared_functions) and their
parameters read from the prototypes, so a new batched entry point is covered without an edit
here as long as it keeps the naming of its neighbours: `mb`, arrays as pointers, `batch`, `ld`,
`stream` (and the rollout's `dt`, `K`, optional `traj`)."""
import ctypes
import re

import pytest

from test_boundary import HEADERS, declared_functions

OK, NULL, ARG, UNSUPPORTED = 0, 1, 2, 6  # rb_status
BATCHED = re.compile(r"^multibody_(\w+?)_batch(_tiled|_host)?_(f32|f64)$")
KIND_MSG = "kind must be 0 rnea, 1 fd, 2 crba, 3 rollout, 4 fwd_kin, 5 jac, 6 rnea_fd, 7 rnea_deriv or 8 fd_deriv"


def _prototypes():
    """{name: [(parameter name, is pointer)]} of every batched entry point the header declares."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADERS[1]).read(), flags=re.S)
    protos = {}
    for name in declared_functions():
        if not BATCHED.match(name):
            continue
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        names = [re.search(r"(\w+)\s*$", p).group(1) for p in params.split(",")]
        protos[name] = [(p, "*" in decl and p != "stream") for p, decl in zip(names, params.split(","))]
    return protos


PROTOS = _prototypes()
NAMES = sorted(PROTOS)


def _op(name):
    return BATCHED.match(name).group(1)


def _form(name):
    return BATCHED.match(name).group(2) or ""


def _arrays(name):
    return [p for p, ptr in PROTOS[name] if ptr and p != "mb"]


def _optional(name):
    """Arrays that may be NULL: the rollout's trajectory, and any (not every) derivative output."""
    op = _op(name)
    if op == "rollout":
        return ["traj"]
    if op.endswith("_deriv"):
        return [a for a in _arrays(name) if a.startswith("d") and "_d" in a or a == "qdd_out"]
    return []


def _inputs(name):
    """Input arrays; the rest of _arrays are outputs (the rollout's state is read and written)."""
    op = _op(name)
    third = {"rnea": "qdd", "fd": "tau", "rnea_deriv": "qdd", "fd_deriv": "tau", "rollout": "tau_seq"}
    ins = {"rnea_fd": ["q", "qd", "qdd", "tau_in"]}.get(op, ["q", "qd", third.get(op)])
    return [a for a in _arrays(name) if a in ins]


class Call:
    """One raw call: every array a distinct dummy buffer unless overridden.  `handle` is never
    combined with arguments that would reach the device."""

    def __init__(self, ffi, name):
        self.ffi, self.name = ffi, name
        self.fn = getattr(ffi.lib(), name)
        self.bufs = {a: (ctypes.c_double * 4)() for a in _arrays(name)}

    def __call__(self, handle, batch, K=1, ld=None, **arrays):
        args = []
        for (p, ptr), ct in zip(PROTOS[self.name], self.fn.argtypes):
            if p == "mb":
                args.append(handle)
            elif ptr:
                buf = arrays.get(p, self.bufs[p]) if "all_null" not in arrays else None
                args.append(None if buf is None else ctypes.cast(buf, ct))
            else:
                args.append({"batch": batch, "ld": batch if ld is None else ld, "stream": None, "dt": 0.01,
                             "K": K}[p])
        return self.fn(*args)


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    return ffi


@pytest.fixture(scope="module")
def fr3(ffi):
    return ffi.Multibody.new()


@pytest.fixture(scope="module")
def tree(ffi):
    """Outside the derivatives' scope (a kinematic tree with general axes)."""
    from rigidbody_amd import chains

    return ffi.Multibody.from_urdf_string(chains.tree_urdf(), ffi.URDF_TREE | ffi.GENERAL_AXES)


def test_header_enumeration():
    """Every family, layout and dtype the header has is in the enumeration."""
    ops = {(_op(n), _form(n)) for n in NAMES}
    for op in ("rnea", "fd", "rnea_fd"):
        assert {(op, ""), (op, "_tiled"), (op, "_host")} <= ops
    for op in ("crba", "fwd_kin", "jac"):
        assert {(op, ""), (op, "_tiled")} <= ops
    assert {("rollout", ""), ("rnea_deriv", ""), ("rnea_deriv", "_host"), ("fd_deriv", ""), ("fd_deriv", "_host")} <= ops
    assert all(n[:-3] + "f32" in PROTOS and n[:-3] + "f64" in PROTOS for n in NAMES)
    for n in NAMES:
        assert [p for p, _ in PROTOS[n]][0] == "mb" and "batch" in [p for p, _ in PROTOS[n]], n
        assert ("ld" in [p for p, _ in PROTOS[n]]) == (_form(n) == ""), n
        assert set(_optional(n)) <= set(_arrays(n)) and len(_inputs(n)) >= 1
    assert _optional("multibody_fd_deriv_batch_f64") == ["qdd_out", "dqdd_dq", "dqdd_dqd", "dqdd_dtau"]
    assert _optional("multibody_rnea_deriv_batch_host_f32") == ["dtau_dq", "dtau_dqd"]


@pytest.mark.parametrize("name", NAMES)
def test_null_handle(ffi, name):
    call = Call(ffi, name)
    for batch in (0, 1, -1):
        assert call(None, batch) == NULL, batch
        assert ffi.last_error() == "NULL Multibody handle"
        assert call(None, batch, all_null=True) == NULL, batch
    assert call(None, 1, K=-1, ld=0) == NULL  # the handle is checked first


@pytest.mark.parametrize("name", NAMES)
def test_negative_batch_and_ld(ffi, fr3, name):
    call = Call(ffi, name)
    for kw in ({}, {"all_null": True}):  # both win over NULL arrays
        assert call(fr3.handle, -1, **kw) == ARG
        assert ffi.last_error() == "negative batch"
        if _form(name) == "":
            assert call(fr3.handle, 1, ld=0, **kw) == ARG
            assert ffi.last_error() == "leading dimension ld < batch"
            assert call(fr3.handle, -1, ld=-2, **kw) == ARG
            assert ffi.last_error() == "negative batch"  # batch before ld


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch(ffi, fr3, tree, name):
    """batch == 0 has nothing to do, whatever the arrays -- and for the derivative forms whatever
    the model: the scope check comes after the empty-batch return."""
    call = Call(ffi, name)
    for mb in (fr3, tree):
        assert call(mb.handle, 0, all_null=True) == OK
        assert call(mb.handle, 0) == OK
        if _form(name) == "":
            assert call(mb.handle, 0, ld=5, all_null=True) == OK


@pytest.mark.parametrize("name", [n for n in NAMES if _op(n) == "rollout"])
def test_rollout_step_count(ffi, fr3, name):
    call = Call(ffi, name)
    for batch in (0, 1):
        assert call(fr3.handle, batch, K=-1) == ARG
        assert ffi.last_error() == "negative step count"
        assert call(fr3.handle, batch, K=-1, all_null=True) == ARG  # before the arrays
        assert call(fr3.handle, batch, K=0, all_null=True) == OK
    assert call(fr3.handle, -1, K=-1) == ARG
    assert ffi.last_error() == "negative batch"  # batch and ld before the step count
    assert call(fr3.handle, 1, K=-1, ld=0) == ARG
    assert ffi.last_error() == "leading dimension ld < batch"


@pytest.mark.parametrize("name", NAMES)
def test_required_arrays(ffi, fr3, name):
    call = Call(ffi, name)
    required = [a for a in _arrays(name) if a not in _optional(name)]
    assert required
    for a in required:
        assert call(fr3.handle, 1, **{a: None}) == NULL, a
        assert ffi.last_error() == "NULL array", a
    assert call(fr3.handle, 1, all_null=True) == NULL


@pytest.mark.parametrize("name", [n for n in NAMES if _op(n) == "rnea_fd" and _form(n) != "_host"])
def test_rnea_fd_aliases(ffi, fr3, name):
    """The device-pointer forms refuse an output that is also an input or the other output (the
    host forms copy into scratch arrays of their own, where nothing can alias)."""
    call = Call(ffi, name)
    for out in ("tau", "qdd_out"):
        for inp in ("q", "qd", "qdd", "tau_in"):
            assert call(fr3.handle, 1, **{out: call.bufs[inp]}) == ARG, (out, inp)
            assert ffi.last_error() == "rnea_fd: an output array is also an input (no in-place form)"
    assert call(fr3.handle, 1, qdd_out=call.bufs["tau"]) == ARG
    assert ffi.last_error() == "rnea_fd: tau and qdd_out are the same array"
    assert call(fr3.handle, 1, tau=None, qdd_out=call.bufs["q"]) == NULL  # NULL arrays first


@pytest.mark.parametrize("name", [n for n in NAMES if _op(n).endswith("_deriv")])
def test_derivative_arrays_and_scope(ffi, fr3, tree, name):
    call = Call(ffi, name)
    op, outs, ins = _op(name), _optional(name), _inputs(name)
    assert len(ins) == 3 and sorted(outs + ins) == sorted(_arrays(name))
    none = {o: None for o in outs}
    for mb in (fr3, tree):  # the array checks come before the model's scope
        assert call(mb.handle, 1, **none) == NULL
        assert ffi.last_error() == f"{op}: every output is NULL"
        assert call(mb.handle, 1, **{**none, ins[0]: None}) == NULL
        assert ffi.last_error() == "NULL array"  # inputs before outputs
        for o in outs:
            for i in ins:
                assert call(mb.handle, 1, **{o: call.bufs[i]}) == ARG, (o, i)
                assert ffi.last_error() == f"{op}: an output array is also an input"
                # ... also when it is the only output
                assert call(mb.handle, 1, **{**none, o: call.bufs[i]}) == ARG, (o, i)
        for k, o in enumerate(outs):
            for o2 in outs[:k]:
                assert call(mb.handle, 1, **{o: call.bufs[o2]}) == ARG, (o, o2)
                assert ffi.last_error() == f"{op}: two outputs are the same array"
    # a model out of scope: refused once the arrays are in order, every output or only one
    assert call(tree.handle, 1) == UNSUPPORTED
    assert "serial revolute" in ffi.last_error()
    assert call(tree.handle, 1, **{**none, outs[-1]: call.bufs[outs[-1]]}) == UNSUPPORTED


def test_fd_deriv_scope_is_the_mass_matrix_form(ffi):
    from rigidbody_amd import chains

    c30 = ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(30))
    for name in NAMES:
        if _op(name) == "fd_deriv":
            assert Call(ffi, name)(c30.handle, 1) == UNSUPPORTED, name
            assert "mass-matrix" in ffi.last_error()
            assert Call(ffi, name)(c30.handle, 0) == OK, name


def test_model_creation_messages(ffi):
    from rigidbody_amd import chains

    lib = ffi.lib()

    def refused(xml, flags=0):
        b = xml.encode()
        assert not lib.multibody_new_from_urdf_string_ex(b, len(b), flags)
        return ffi.last_error()

    x_axis = chains.synthetic_chain_urdf(3).replace('<axis xyz="0 0 1"/>', '<axis xyz="1 0 0"/>', 1)
    assert refused(x_axis) == ("non-z joint axis: the reference injects joint motion about local z "
                               "(multibody.rs:130-138,144); pass RB_MODEL_GENERAL_AXES for general axes")
    bad = next(k for k in range(1, 64) if k not in ffi.supported_dofs())
    assert refused(chains.synthetic_chain_urdf(bad)) == f"no kernel compiled for {bad} DOF"
    # a prismatic joint makes a chain a "tree" model for the kernels: any DOF up to 64
    long = chains.synthetic_chain_urdf(65).replace('type="revolute"', 'type="prismatic"', 1)
    assert 'type="prismatic"' in long
    assert refused(long, ffi.URDF_TREE) == "tree models support at most 64 DOF, got 65"


def test_kernel_inspection_argument_errors(ffi, fr3, tree):
    lib = ffi.lib()
    buf = ctypes.create_string_buffer(b"x" * 15, 16)
    queries = (lambda *a: lib.multibody_kernel_path_ex(*a), lambda *a: lib.multibody_kernel_form_ex(*a),
               lambda *a: lib.multibody_jit_source_ex(*a, buf, 16))
    for query in queries:
        assert query(None, 0, 0, 1, 0) == -NULL
        assert ffi.last_error() == "NULL Multibody handle"
        for kind in (-1, 9):
            assert query(fr3.handle, kind, 0, 1 << 20, 0) == -ARG, kind
            assert ffi.last_error() == KIND_MSG
        for batch in (0, -1):
            assert query(fr3.handle, 0, 1, batch, 0) == -ARG, batch
            assert ffi.last_error() == "batch must be positive"
        assert query(fr3.handle, 9, 0, 0, 0) == -ARG
        assert ffi.last_error() == KIND_MSG  # the kind before the batch
    # a derivative kind outside its scope: refused by the path / form queries, the empty source
    for kind in (7, 8):
        assert lib.multibody_kernel_path_ex(tree.handle, kind, 1, 1 << 20, 0) == -UNSUPPORTED
        assert "serial revolute" in ffi.last_error()
        assert lib.multibody_kernel_form_ex(tree.handle, kind, 0, 1, 0) == -UNSUPPORTED
        buf.raw = b"x" * 16
        assert lib.multibody_jit_source_ex(tree.handle, kind, 1, 1 << 20, 0, buf, 16) == 0
        assert buf.raw[0] == 0  # the empty source, NUL-terminated
        assert lib.multibody_jit_source_ex(tree.handle, kind, 1, 1 << 20, 0, None, 0) == 0
        assert lib.multibody_jit_compile_ex(tree.handle, kind, 1, 1 << 20, 0, None) == -UNSUPPORTED
    assert lib.multibody_jit_compile_ex(fr3.handle, 9, 0, 1, 0, None) == -ARG
