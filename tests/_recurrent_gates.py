"""Shared by the gate-pass tests of ``csrc/gru.hip`` (tests/test_recurrent_gates.py on the CPU, test_recurrent_gates_gpu.py on
the device): the cases (seeded inputs, shapes, scales), the float64 references (``oracle``), the assertions, and a float32
numpy restatement of the same arithmetic — fp32 at every intermediate — that the CPU test runs through those very assertions:
the evidence, obtainable without a GPU, that correct fp32 code stays inside the bounds the device is held to.

A backend (``F32`` here, the device one in the GPU test) takes a case's operands as numpy arrays and returns what the launch
wrote, as numpy arrays; ``exercise`` runs one case through a backend and asserts."""

from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

import oracle

GATES = {"gru": 3, "lstm": 4, "rnn": 1}
FAMILY = {"gru": "gru_gates", "lstm": "lstm_gates", "rnn": "rnn_cell"}
BLOCK = 256  # threads per block of every gate pass
BIAS_ROWS = (0, 4, 8, 16, 32)  # the values of the `gru_bias_rows` option (0: the kernel's own rule, 16)
BIAS_WIDTHS = (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 12, 5)
SATURATION = (20.0, 90.0, 1e4)


@dataclass(frozen=True)
class Case:
    name: str
    cell: str
    B: int
    H: int
    t: int = 2
    lengths: str = "none"  # none | mixed | ended | live
    b_hh: bool = True
    d_out: bool = True
    scale: float = 1.0
    garbage: bool = False  # NaN in whatever a launch may not read of an ended row
    saturated: bool = False
    relu: bool = False
    save: bool = True  # LSTM forward: the training form (c_saved given)
    rows: int = 0  # bias-folding pass: rows per block (0: the plain pass)
    form: str = "vec"  # bias-folding pass: 16-byte lanes | scalar (forced by an operand one float off alignment)


def _lengths(case: Case):
    """Per-row lengths around ``t``: rows with t < len - 1, t == len - 1, t == len and t > len, in turn."""
    t, B = case.t, case.B
    if case.lengths == "none":
        return None
    if case.lengths == "ended":
        return np.array([(0, t, max(t - 1, 0))[b % 3] for b in range(B)], np.int64)
    if case.lengths == "live":
        return np.array([(t + 1, t + 5)[b % 2] for b in range(B)], np.int64)
    return np.array([(t + 3, t + 1, t, max(t - 1, 0))[b % 4] for b in range(B)], np.int64)


def inputs(case: Case) -> dict:
    """Every operand of the case's forward and backward launches: float32 arrays (``None`` for an absent optional one),
    ``lengths`` int64 or None.  The backward operands are consistent with the forward ones (LSTM ``pre`` / ``c_next`` and the
    RNN's ``out`` are what the forward step saves)."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    B, H, G = case.B, case.H, GATES[case.cell]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    gi, gh = rng.standard_normal((B, G * H)) * case.scale, rng.standard_normal((B, G * H)) * case.scale
    h, c = rng.standard_normal((B, H)), rng.standard_normal((B, H))
    if case.saturated:
        # row k saturates ONE gate: pre-activation +-20 | 90 | 1e4, carried by gi in the even columns and by gh in the odd
        # ones; states of magnitude up to 50 in the second half of the rows
        for k in range(B):
            gate, rest = k % G, k // G
            value = SATURATION[rest % 3] * (1.0 if (rest // 3) % 2 == 0 else -1.0)
            columns = np.arange(H)
            gi[k, gate * H + columns[columns % 2 == 0]] = value
            gh[k, gate * H + columns[columns % 2 == 1]] = value
            if k >= B // 2:
                h[k] *= 25.0
                c[k] *= 25.0
        h, c = np.clip(h, -50.0, 50.0), np.clip(c, -50.0, 50.0)
    data = {"gi": f32(gi), "gh": f32(gh), "b_hh": f32(rng.standard_normal(G * H) * 0.5) if case.b_hh else None,
            "h": f32(h), "dh": f32(rng.standard_normal((B, H))), "d_out": f32(rng.standard_normal((B, H))) if case.d_out else None,
            "lengths": _lengths(case), "t": case.t}
    if case.cell == "lstm":
        data["c"], data["dc"] = f32(c), f32(rng.standard_normal((B, H)))
        _, c_next, _, pre, _ = oracle.lstm_gates_step(data["gi"], data["gh"], data["b_hh"], data["h"], data["c"], data["lengths"], case.t)
        data["pre"], data["c_next"] = f32(pre), f32(c_next)
    if case.cell == "rnn":
        data["y"] = f32(oracle.rnn_cell_step(data["gi"], data["gh"], data["b_hh"], data["h"], data["lengths"], case.t, case.relu)[1])
    if case.garbage and data["lengths"] is not None:
        dead = case.t >= data["lengths"]
        for name in ("gi", "gh", "pre", "c_next", "y"):
            if name in data:
                data[name][dead] = np.nan
        # for the backward launch only (the forward pass keeps the state of an ended row, so that one must be finite there)
        data["garbage"] = {"gru": ("h",), "rnn": (), "lstm": ("c",)}[case.cell]
    return data


def backward_operands(data: dict) -> dict:
    """The operands as the BACKWARD launch sees them: the saved states of ended rows hold NaN in a ``garbage`` case."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    if "garbage" in data:
        dead = data["t"] >= data["lengths"]
        for name in data["garbage"]:
            out[name][dead] = np.nan
    return out


# ------------------------------------------------------------------------------------------------ the cases
def plain_cases(cell: str) -> list[Case]:
    cases = []

    def add(tag, B, H, **kw):
        for relu in ((False, True) if cell == "rnn" else (False,)):
            cases.append(Case(f"{cell}{'_relu' if relu else ''}/{tag}/B{B}H{H}", cell, B, H, relu=relu, **kw))

    # lanes (H = 8), scalar (H = 5, 7), H = 1, B = 1; B * cols = 255, 256, 257 threads and their neighbours
    for B, H in ((6, 8), (6, 5), (6, 7), (3, 1), (50, 5), (51, 5), (52, 5), (63, 16), (64, 16), (65, 16), (256, 4), (257, 4), (258, 4)):
        add("shape", B, H, lengths="mixed", garbage=True)
    for H in (8, 5):
        add("one_row", 1, H)
        add("one_row_ended", 1, H, lengths="ended", garbage=True)
        for i, (b_hh, d_out, lengths) in enumerate((b, d, l) for b in (True, False) for d in (True, False) for l in ("none", "mixed")):
            add(f"operands_b{int(b_hh)}d{int(d_out)}_{lengths}", 6, H, b_hh=b_hh, d_out=d_out, lengths=lengths, scale=(1.0, 4.0)[i % 2])
        add("all_ended", 6, H, lengths="ended", garbage=True)
        add("all_live", 6, H, lengths="live")
        add("t0", 6, H, t=0, lengths="mixed", garbage=True)
        add("t23", 6, H, t=23, lengths="mixed", garbage=True, scale=4.0)
        if cell == "lstm":
            add("eval", 6, H, save=False, lengths="mixed", garbage=True)
            add("eval_plain", 6, H, save=False)
    if cell == "lstm":
        add("eval", 51, 5, save=False, lengths="mixed")
    # every gate x magnitude x sign once (a second time with large states)
    rows = 2 * GATES[cell] * 6
    add("saturated", rows, 8, saturated=True)
    add("saturated", rows, 5, saturated=True, lengths="mixed", garbage=True)
    add("saturated_bare", rows, 8, saturated=True, b_hh=False, d_out=False)
    return cases


PLAIN = {cell: plain_cases(cell) for cell in GATES}


def effective_rows(rows: int) -> int:
    return rows or 16


def bias_eligible(rows: int, H: int, form: str) -> bool:
    """The rule of ``cusrl_gru_bias_supported``, written out: the column chunks of a row (H / 4 lanes of 16 bytes, H scalars)
    tile a 256-thread block, and the rows the block then has in flight fit into the rows it owns."""
    cols = H // 4 if form == "vec" and H % 4 == 0 else H
    return BLOCK % cols == 0 and BLOCK // cols <= effective_rows(rows)


def bias_cases(rows: int) -> list[Case]:
    cases = []
    own = effective_rows(rows)
    for H in BIAS_WIDTHS:
        for form in ("vec", "scalar"):
            if (form == "vec" and H % 4) or not bias_eligible(rows, H, form):
                continue
            for B in sorted({1, own - 1, own, own + 1, 3 * own + 2}):
                for lengths in ("none", "mixed"):
                    for b_hh in (True, False):
                        for d_out in (True, False):
                            cases.append(Case(f"gru/bias{rows}_{form}_b{int(b_hh)}d{int(d_out)}_{lengths}/B{B}H{H}", "gru", B, H,
                                              lengths=lengths, garbage=lengths != "none", b_hh=b_hh, d_out=d_out,
                                              scale=(1.0, 4.0)[B % 2], rows=own, form=form))
    return cases


# ------------------------------------------------------------------------------------------------ fp32 restatement
class F32:
    """The gate passes in numpy float32, every intermediate rounded to fp32 (no fused multiply-add: the library is built with
    contraction off).  Same results as the float64 references up to rounding; the bias partials are accumulated in the
    kernel's order (a thread sums its rows, the block folds its row groups, group 0 first)."""

    one = np.float32(1.0)

    @classmethod
    def sigmoid(cls, v):
        with np.errstate(over="ignore"):
            return cls.one / (cls.one + np.exp(-v))

    @staticmethod
    def live(data, B):
        return (np.ones(B, bool) if data["lengths"] is None else data["t"] < data["lengths"])[:, None]

    @staticmethod
    def bias(data, n):
        return np.zeros(n, np.float32) if data["b_hh"] is None else data["b_hh"]

    @classmethod
    def forward(cls, case: Case, data: dict) -> dict:
        with np.errstate(invalid="ignore", over="ignore"):
            return getattr(cls, case.cell + "_forward")(case, data)

    @classmethod
    def backward(cls, case: Case, data: dict) -> dict:
        with np.errstate(invalid="ignore", over="ignore"):
            return getattr(cls, case.cell + "_backward")(case, data)

    @classmethod
    def gru_gates(cls, data, h):
        H = h.shape[1]
        gi, gh, b = data["gi"], data["gh"], cls.bias(data, 3 * H)
        r = cls.sigmoid(gi[:, :H] + gh[:, :H] + b[:H])
        z = cls.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H] + b[H:2 * H])
        q = gh[:, 2 * H:] + b[2 * H:]
        n = np.tanh(gi[:, 2 * H:] + r * q)
        return r, z, q, n

    @classmethod
    def gru_forward(cls, case, data):
        h = data["h"]
        r, z, q, n = cls.gru_gates(data, h)
        nxt = (cls.one - z) * n + z * h
        live = cls.live(data, case.B)
        return {"h": np.where(live, nxt, h), "out": np.where(live, nxt, np.float32(0.0))}

    @classmethod
    def gru_backward(cls, case, data):
        h, dh = data["h"], data["dh"]
        r, z, q, n = cls.gru_gates(data, h)
        upstream = dh if data["d_out"] is None else dh + data["d_out"]
        d_n = upstream * (cls.one - z) * (cls.one - n * n)
        d_q = d_n * r
        d_r = d_n * q * r * (cls.one - r)
        d_z = upstream * (h - n) * z * (cls.one - z)
        live = cls.live(data, case.B)
        d_r, d_z, d_n, d_q = (np.where(live, d, np.float32(0.0)) for d in (d_r, d_z, d_n, d_q))
        got = {"gi": np.concatenate([d_r, d_z, d_n], 1), "gh": np.concatenate([d_r, d_z, d_q], 1), "dh": np.where(live, upstream * z, dh)}
        if case.rows:
            got["bias_partials"] = cls.bias_partials(case, np.concatenate([d_r, d_z, d_n, d_q], 1))
        return got

    @staticmethod
    def bias_partials(case, terms):
        """``terms`` [B, 4H]: what the pass wrote (zeros for ended rows).  A block owns ``rows`` consecutive rows; thread group g
        of ``groups`` = 256 / cols sums rows g, g + groups, ... in that order, then the groups are summed, group 0 first."""
        B, width = terms.shape
        cols = case.H // 4 if case.form == "vec" else case.H
        groups, rows = BLOCK // cols, case.rows
        blocks = -(-B // rows)
        padded = np.zeros((blocks * rows, width), np.float32)
        padded[:B] = terms
        padded = padded.reshape(blocks, rows // groups, groups, width)
        acc = np.zeros((blocks, groups, width), np.float32)
        for p in range(rows // groups):
            acc = acc + padded[:, p]
        total = np.zeros((blocks, width), np.float32)
        for g in range(groups):
            total = total + acc[:, g]
        return total

    @classmethod
    def lstm_forward(cls, case, data):
        h, c = data["h"], data["c"]
        H = h.shape[1]
        pre = data["gi"] + data["gh"] + cls.bias(data, 4 * H)
        i, f, g, o = cls.sigmoid(pre[:, :H]), cls.sigmoid(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), cls.sigmoid(pre[:, 3 * H:])
        c_new = f * c + i * g
        h_new = o * np.tanh(c_new)
        live = cls.live(data, case.B)
        got = {"h": np.where(live, h_new, h), "c": np.where(live, c_new, c), "out": np.where(live, h_new, np.float32(0.0))}
        got["gi"] = pre if case.save else data["gi"].copy()
        if case.save:
            got["c_saved"] = got["c"].copy()
        return got

    @classmethod
    def lstm_backward(cls, case, data):
        pre, dh, dc = data["pre"], data["dh"], data["dc"]
        H = dh.shape[1]
        i, f, g, o = cls.sigmoid(pre[:, :H]), cls.sigmoid(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), cls.sigmoid(pre[:, 3 * H:])
        tc = np.tanh(data["c_next"])
        upstream = dh if data["d_out"] is None else dh + data["d_out"]
        d_c = dc + upstream * o * (cls.one - tc * tc)
        d_pre = np.concatenate([d_c * g * i * (cls.one - i), d_c * data["c"] * f * (cls.one - f), d_c * i * (cls.one - g * g),
                                upstream * tc * o * (cls.one - o)], 1)
        live = cls.live(data, case.B)
        zero = np.float32(0.0)
        return {"pre": np.where(live, d_pre, zero), "dh": np.where(live, zero, dh), "dc": np.where(live, d_c * f, dc)}

    @classmethod
    def rnn_forward(cls, case, data):
        h = data["h"]
        pre = data["gi"] + data["gh"] + cls.bias(data, h.shape[1])
        nxt = np.maximum(pre, np.float32(0.0)) if case.relu else np.tanh(pre)
        live = cls.live(data, case.B)
        return {"h": np.where(live, nxt, h), "out": np.where(live, nxt, np.float32(0.0))}

    @classmethod
    def rnn_backward(cls, case, data):
        y, dh = data["y"], data["dh"]
        upstream = dh if data["d_out"] is None else dh + data["d_out"]
        zero = np.float32(0.0)
        d_pre = np.where(y > zero, upstream, zero) if case.relu else upstream * (cls.one - y * y)
        live = cls.live(data, case.B)
        return {"d_pre": np.where(live, d_pre, zero), "dh": np.where(live, zero, dh)}


# ------------------------------------------------------------------------------------------------ references
def reference_forward(case: Case, data: dict) -> dict:
    d, args = data, (data["lengths"], data["t"])
    if case.cell == "gru":
        h, out = oracle.gru_gates_step(d["gi"], d["gh"], d["b_hh"], d["h"], *args)
        return {"h": h, "out": out}
    if case.cell == "rnn":
        h, out = oracle.rnn_cell_step(d["gi"], d["gh"], d["b_hh"], d["h"], *args, case.relu)
        return {"h": h, "out": out}
    h, c, out, pre, c_saved = oracle.lstm_gates_step(d["gi"], d["gh"], d["b_hh"], d["h"], d["c"], *args)
    want = {"h": h, "c": c, "out": out}
    if case.save:
        want["gi"], want["c_saved"] = pre, c_saved
    return want


def reference_backward(case: Case, data: dict) -> dict:
    d, args = data, (data["lengths"], data["t"])
    if case.cell == "gru":
        d_gi, d_gh, dh, sums = oracle.gru_gates_step_backward(d["gi"], d["gh"], d["b_hh"], d["h"], d["d_out"], d["dh"], *args)
        return {"gi": d_gi, "gh": d_gh, "dh": dh, "column_sums": sums}
    if case.cell == "rnn":
        d_pre, dh = oracle.rnn_cell_step_backward(d["y"], d["d_out"], d["dh"], *args, case.relu)
        return {"d_pre": d_pre, "dh": dh}
    d_pre, dh, dc = oracle.lstm_gates_step_backward(d["pre"], d["c"], d["c_next"], d["d_out"], d["dh"], d["dc"], *args)
    return {"pre": d_pre, "dh": dh, "dc": dc}


# ------------------------------------------------------------------------------------------------ assertions
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _saturated_bound(label, got, want):
    """A saturated case: finite, and within 1e-5 of max(1, the tensor's largest entry) — absolute, because whole tensors are
    ~0 there (d_z at pre-activation 90 is 1e-39 in float64 and 0 in fp32: no relative measure applies)."""
    assert np.isfinite(got).all(), f"{label}: not finite"
    error, scale = float(np.abs(got.astype(np.float64) - want).max()), max(1.0, float(np.abs(want).max()))
    print(f"{label}: |got - want| = {error:.3e}, bound {1e-5 * scale:.3e}")
    assert error <= 1e-5 * scale, f"{label}: |got - want| = {error:.3e} exceeds 1e-5 * {scale:.3e}"


def _dead(data):
    return None if data["lengths"] is None else data["t"] >= data["lengths"]


def check_forward(case: Case, data: dict, got: dict) -> None:
    want = reference_forward(case, data)
    assert set(want) <= set(got), (sorted(want), sorted(got))
    for name, reference in want.items():
        label = f"{case.name}:{name}"
        assert got[name].shape == reference.shape and got[name].dtype == np.float32, label
        if case.saturated:
            live = np.isfinite(reference)  # (the saved pre-activations of an ended row are what its gi / gh rows held)
            assert np.array_equal(np.isnan(got[name]), ~live), label
            _saturated_bound(label, got[name][live], reference[live])
        else:
            np.testing.assert_allclose(got[name], reference, rtol=1e-5, atol=2e-6, err_msg=label)
    dead = _dead(data)
    if dead is not None:  # bitwise: the state of an ended row is kept, its output is zero
        assert same_bits(got["h"][dead], data["h"][dead]), f"{case.name}: h of an ended row changed"
        assert not _bits(got["out"][dead]).any(), f"{case.name}: out of an ended row is not zero"
        if case.cell == "lstm":
            assert same_bits(got["c"][dead], data["c"][dead]), f"{case.name}: c of an ended row changed"
            if case.save:
                assert same_bits(got["c_saved"][dead], data["c"][dead]), f"{case.name}: c_saved of an ended row"
    if case.cell == "lstm" and not case.save:
        assert same_bits(got["gi"], data["gi"]), f"{case.name}: the eval form wrote into gi"


GRADIENTS = {"gru": ("gi", "gh", "dh"), "lstm": ("pre", "dh", "dc"), "rnn": ("d_pre", "dh")}
GATE_GRADIENTS = {"gru": ("gi", "gh"), "lstm": ("pre",), "rnn": ("d_pre",)}


def check_backward(case: Case, data: dict, got: dict, parity, family: str | None = None) -> dict:
    """``data``: the operands of the backward launch (``backward_operands``).  Returns the float64 reference."""
    family = family or FAMILY[case.cell]
    want = reference_backward(case, data)
    for name in GRADIENTS[case.cell]:
        label = f"{family}[{case.name}:{name if name.startswith('d') else 'd_' + name}]"
        assert got[name].shape == want[name].shape and got[name].dtype == np.float32, label
        if case.saturated:
            _saturated_bound(label, got[name], want[name])
        else:
            parity(label, got[name], want[name], 1e-5)
    dead = _dead(data)
    if dead is not None:  # bitwise: no gate gradient for an ended row, its state gradient passes through
        for name in GATE_GRADIENTS[case.cell]:
            assert not _bits(got[name][dead]).any(), f"{case.name}: d_{name} of an ended row is not zero"
        for name in ("dh", "dc")[: 2 if case.cell == "lstm" else 1]:
            assert same_bits(got[name][dead], data[name][dead]), f"{case.name}: {name} of an ended row changed"
    return want


def check_bias_partials(case: Case, data: dict, got: dict, want: dict) -> None:
    """The partial rows of the bias-folding pass: their count, their total (the soak test's rule for bias gradients: 1e-5 of the
    largest column's sum of |terms|) and block ownership — partial row k is the sum of rows [k * rows, (k + 1) * rows) of what
    the SAME launch wrote, to fp32 summation accuracy: a row that is dropped, counted twice or credited to a neighbouring block
    can leave the total intact."""
    B, H, rows = case.B, case.H, case.rows
    partials = got["bias_partials"]
    blocks = -(-B // rows)
    assert partials.shape == (blocks, 4 * H), (case.name, partials.shape)
    assert np.isfinite(partials).all(), f"{case.name}: a bias partial is not finite"
    # reference terms of the live rows {d_r, d_z, d_n, d_q}: |terms| summed per column
    terms = np.concatenate([want["gi"], want["gh"][:, 2 * H:]], 1)
    magnitude = float(np.abs(terms).sum(0).max())
    error = float(np.abs(partials.astype(np.float64).sum(0) - want["column_sums"]).max())
    print(f"{case.name}: column sums off by {error:.3e}, bound {1e-5 * magnitude:.3e}")
    assert error <= 1e-5 * magnitude, f"{case.name}: bias column sums off by {error:.3e} > 1e-5 * {magnitude:.3e}"
    written = np.concatenate([got["gi"], got["gh"][:, 2 * H:]], 1).astype(np.float64)
    for k in range(blocks):
        block = written[k * rows:(k + 1) * rows]
        bound = rows * 2.0 ** -23 * np.abs(block).sum(0)
        off = np.abs(partials[k].astype(np.float64) - block.sum(0))
        assert (off <= bound).all(), (f"{case.name}: partial row {k} is not the sum of rows [{k * rows}, {min((k + 1) * rows, B)}) "
                                      f"of the gradients the launch wrote (column {int(np.argmax(off - bound))}: off by {off.max():.3e})")


def exercise(case: Case, backend, parity, family: str | None = None) -> None:
    """One case through a backend: the forward launch, then the backward launch, each against float64."""
    data = inputs(case)
    check_forward(case, data, backend.forward(case, data))
    operands = backward_operands(data)
    got = backend.backward(case, operands)
    want = check_backward(case, operands, got, parity, family)
    if case.rows:
        check_bias_partials(case, operands, got, want)
