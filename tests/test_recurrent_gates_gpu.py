"""The nine launch entry points of ``csrc/gru.hip`` — GRU forward / backward / backward with folded bias sums, LSTM and RNN
forward / backward, each in its 16-byte-lane and its scalar form — called directly (``ops.gru_gates_*``, ``ops.lstm_gates_*``,
``ops.rnn_cell_*``) and held to the float64 single-step references of ``oracle``.  The cases, references and assertions are
those of tests/_recurrent_gates.py; tests/test_recurrent_gates.py runs the same cases through a float32 restatement and the same
assertions without a GPU.  Bounds (the project's standing ones): forward 1e-5 relative + 2e-6; every gradient tensor 1e-5 of its
largest entry (``gradient_parity``); saturated cases finite and within 1e-5 * max(1, largest entry); ended rows bitwise."""

import dataclasses
import zlib

import numpy as np
import pytest
import torch

import _recurrent_gates as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4  # floats behind every operand that no launch may touch
SENTINEL = -1234.5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from cusrl_amd import ops as _ops

    return _ops


@pytest.fixture
def option():
    """``option(key, value)``: ``cusrl_set_option`` for the duration of the test (every key it touched goes back to 0 — the kernel's
    own rule — afterwards)."""
    from cusrl_amd import _native

    touched = []

    def set_(key, value):
        touched.append(key)
        _native.set_option(key, value)
        assert _native.get_option(key) == value

    yield set_
    for key in touched:
        _native.set_option(key, 0)


class Device:
    """The backend of ``G.exercise`` on the GPU.  Every operand is a fresh device copy inside an allocation of its own with
    guard floats behind it (``offset``: the named operand starts one float into its allocation — not 16-byte aligned — which
    sends an H % 4 == 0 launch to the scalar form); after the launch the guards and the read-only operands must be untouched."""

    def __init__(self, ops, offset: str | None = None):
        self.ops, self.offset = ops, offset

    def begin(self):
        self.placed = {}

    def place(self, name, array, shape=None, guard=GUARD):
        """Device view of ``array`` (or an output of ``shape`` filled with NaN: every element has to be written)."""
        if array is None and shape is None:
            return None
        shape = tuple(array.shape) if shape is None else shape
        lead = 1 if name == self.offset else 0
        buffer = torch.full((lead + int(np.prod(shape)) + guard,), SENTINEL, dtype=torch.float32, device=DEV)
        view = buffer[lead:lead + int(np.prod(shape))].view(shape)
        view.copy_(torch.from_numpy(array)) if array is not None else view.fill_(float("nan"))
        assert view.is_contiguous() and view.data_ptr() % 16 == (4 if lead else 0)
        self.placed[name] = (buffer, view, lead, guard, None if array is None else array.copy())
        return view

    def lengths(self, data):
        return None if data["lengths"] is None else torch.from_numpy(data["lengths"]).to(DEV)

    def finish(self, written: dict[str, str], read_only) -> dict:
        """``written``: {result name: operand name}.  Checks guards and read-only operands, returns the results on the host."""
        torch.cuda.synchronize()
        for name, (buffer, view, lead, guard, original) in self.placed.items():
            host = buffer.cpu().numpy()
            assert (host[:lead] == SENTINEL).all() and (host[host.size - guard:] == SENTINEL).all(), f"{name}: wrote out of bounds"
            if name in read_only and original is not None:
                assert G.same_bits(view.cpu().numpy(), original), f"{name}: a read-only operand changed"
        return {result: self.placed[name][1].cpu().numpy() for result, name in written.items()}

    def forward(self, case, d):
        self.begin()
        ops, B, H = self.ops, case.B, case.H
        gi, gh, b_hh, h = (self.place(n, d[n]) for n in ("gi", "gh", "b_hh", "h"))
        out = self.place("out", None, (B, H))
        if case.cell == "gru":
            ops.gru_gates_forward(gi, gh, b_hh, h, out, self.lengths(d), d["t"])
            return self.finish({"h": "h", "out": "out"}, ("gi", "gh", "b_hh"))
        if case.cell == "rnn":
            ops.rnn_cell_forward(gi, gh, b_hh, h, out, self.lengths(d), d["t"], case.relu)
            return self.finish({"h": "h", "out": "out"}, ("gi", "gh", "b_hh"))
        c = self.place("c", d["c"])
        c_saved = self.place("c_saved", None, (B, H)) if case.save else None
        ops.lstm_gates_forward(gi, gh, b_hh, h, c, out, c_saved, self.lengths(d), d["t"])
        written = {"h": "h", "c": "c", "out": "out", "gi": "gi"}
        if case.save:
            written["c_saved"] = "c_saved"
        return self.finish(written, ("gh", "b_hh") + (() if case.save else ("gi",)))

    def backward(self, case, d):
        self.begin()
        ops, B, H = self.ops, case.B, case.H
        d_out, dh = self.place("d_out", d["d_out"]), self.place("dh", d["dh"])
        if case.cell == "gru":
            gi, gh, b_hh, h = (self.place(n, d[n]) for n in ("gi", "gh", "b_hh", "h"))
            written = {"gi": "gi", "gh": "gh", "dh": "dh"}
            partials = None
            if case.rows:
                blocks = ops.gru_bias_partial_rows(B)
                assert blocks == -(-B // case.rows)
                partials = self.place("bias_partials", None, (blocks, 4 * H), guard=4 * H)  # a whole guard row behind the last one
                written["bias_partials"] = "bias_partials"
                assert ops.gru_bias_partials_supported(H, gi, gh, b_hh, h, d_out, dh, partials)
            ops.gru_gates_backward(gi, gh, b_hh, h, d_out, dh, self.lengths(d), d["t"], partials)
            return self.finish(written, ("b_hh", "h", "d_out"))
        if case.cell == "rnn":
            d_pre, y = self.place("d_pre", None, (B, H)), self.place("y", d["y"])
            ops.rnn_cell_backward(d_pre, y, d_out, dh, self.lengths(d), d["t"], case.relu)
            return self.finish({"d_pre": "d_pre", "dh": "dh"}, ("y", "d_out"))
        pre, c, c_next, dc = (self.place(n, d[n]) for n in ("pre", "c", "c_next", "dc"))
        ops.lstm_gates_backward(pre, c, c_next, d_out, dh, dc, self.lengths(d), d["t"])
        return self.finish({"pre": "pre", "dh": "dh", "dc": "dc"}, ("c", "c_next", "d_out"))


FORWARD_OPERANDS = {"gru": ("gi", "gh", "b_hh", "h", "out"), "rnn": ("gi", "gh", "b_hh", "h", "out"),
                    "lstm": ("gi", "gh", "b_hh", "h", "c", "out", "c_saved")}
BACKWARD_OPERANDS = {"gru": ("gi", "gh", "b_hh", "h", "d_out", "dh"), "rnn": ("d_pre", "y", "d_out", "dh"),
                     "lstm": ("pre", "c", "c_next", "d_out", "dh", "dc")}


@pytest.mark.parametrize("case", [case for cell in G.GATES for case in G.PLAIN[cell]], ids=lambda case: case.name)
def test_gate_pass_against_float64(ops, case, gradient_parity):
    """Forward and backward launch of one case: lanes and scalar widths, partial last blocks, every optional operand absent and
    given, lengths that end rows before, at and after ``t`` (NaN in what an ended row's launch may not read), saturated gates."""
    from cusrl_amd import _native

    names = {"gru": ("cusrl_gru_gates_fwd", "cusrl_gru_gates_bwd"), "lstm": ("cusrl_lstm_gates_fwd", "cusrl_lstm_gates_bwd"),
             "rnn": ("cusrl_rnn_cell_fwd", "cusrl_rnn_cell_bwd")}[case.cell]
    before = [_native.launch_counts.get(name, 0) for name in names]
    G.exercise(case, Device(ops), gradient_parity)
    assert [_native.launch_counts.get(name, 0) for name in names] == [count + 1 for count in before]


@pytest.mark.parametrize("cell", list(G.GATES))
def test_a_misaligned_operand_takes_the_scalar_form_bit_for_bit(ops, cell, gradient_parity):
    """H = 8 with, in turn, each pointer operand one float off 16-byte alignment: the launch must take the scalar form (a lane
    access there is a misaligned 16-byte access) and give the bits of the aligned run, which is itself held to float64."""
    for relu in ((False, True) if cell == "rnn" else (False,)):
        case = G.Case(f"{cell}{'_relu' if relu else ''}/offset/B6H8", cell, 6, 8, lengths="mixed", garbage=True, relu=relu)
        data = G.inputs(case)
        operands = G.backward_operands(data)
        forward, backward = Device(ops).forward(case, data), Device(ops).backward(case, operands)
        G.check_forward(case, data, forward)
        G.check_backward(case, operands, backward, gradient_parity)
        for name in FORWARD_OPERANDS[cell]:
            got = Device(ops, offset=name).forward(case, data)
            assert all(G.same_bits(got[key], forward[key]) for key in forward), (cell, "forward", name)
        for name in BACKWARD_OPERANDS[cell]:
            got = Device(ops, offset=name).backward(case, operands)
            assert all(G.same_bits(got[key], backward[key]) for key in backward), (cell, "backward", name)


def test_an_empty_batch_launches_nothing(ops):
    """B = 0: every entry point returns without touching anything (and without looking at its pointers)."""
    H = 8
    buffer = torch.full((64,), SENTINEL, device=DEV)
    empty = lambda width: buffer[8:8].view(0, width)  # noqa: E731
    lengths = torch.zeros(0, dtype=torch.int64, device=DEV)
    wide, tall, state = empty(3 * H), empty(4 * H), empty(H)
    ops.gru_gates_forward(wide, wide, None, state, state, lengths, 0)
    ops.gru_gates_backward(wide, wide, None, state, None, state, lengths, 0)
    ops.gru_gates_backward(wide, wide, None, state, None, state, lengths, 0, empty(4 * H))
    ops.lstm_gates_forward(tall, tall, None, state, state, state, state, lengths, 0)
    ops.lstm_gates_backward(tall, state, state, None, state, state, lengths, 0)
    for relu in (False, True):
        ops.rnn_cell_forward(state, state, None, state, state, lengths, 0, relu)
        ops.rnn_cell_backward(state, state, None, state, lengths, 0, relu)
    torch.cuda.synchronize()
    assert bool((buffer == SENTINEL).all()) and ops.gru_bias_partial_rows(0) == 0


def _scalar_offset(case) -> str:
    """Which operand of a scalar-form bias launch is the misaligned one: the partial rows or, in turn, a gate operand."""
    return ("bias_partials", "dh", "gi", "h")[zlib.crc32(case.name.encode()) % 4]


@pytest.mark.parametrize("rows", G.BIAS_ROWS)
def test_bias_folding_eligibility_is_the_written_rule(ops, option, rows):
    """``gru_bias_partials_supported`` == (cols | 256 and 256 / cols <= rows, cols = H / 4 in lanes, H in scalars) for every
    ``gru_bias_rows`` and width, and the launch agrees with it: it runs exactly where the predicate says yes, and where it says
    no it reports CUSRL_E_UNSUPPORTED and leaves every operand as it was."""
    from cusrl_amd import _native

    option("gru_bias_rows", rows)
    own = G.effective_rows(rows)
    for H in G.BIAS_WIDTHS:
        for form in ("vec", "scalar"):
            cols = H // 4 if form == "vec" and H % 4 == 0 else H
            rule = 256 % cols == 0 and 256 // cols <= own
            assert rule == G.bias_eligible(rows, H, form)
            case = G.Case(f"gru/eligibility{rows}_{form}/B3H{H}", "gru", 3, H, lengths="mixed", rows=own, form=form)
            data = G.backward_operands(G.inputs(case))
            device = Device(ops, offset=_scalar_offset(case) if form == "scalar" else None)
            device.begin()
            gi, gh, b_hh, h, d_out, dh = (device.place(n, data[n]) for n in ("gi", "gh", "b_hh", "h", "d_out", "dh"))
            assert ops.gru_bias_partial_rows(3) == 1
            partials = device.place("bias_partials", None, (1, 4 * H), guard=4 * H)
            assert ops.gru_bias_partials_supported(H, gi, gh, b_hh, h, d_out, dh, partials) == rule, (rows, H, form)
            before = _native.launch_counts.get("cusrl_gru_gates_bwd_bias", 0)
            if rule:
                ops.gru_gates_backward(gi, gh, b_hh, h, d_out, dh, device.lengths(data), data["t"], partials)
                got = device.finish({"gi": "gi", "gh": "gh", "dh": "dh", "bias_partials": "bias_partials"}, ("b_hh", "h", "d_out"))
                assert np.isfinite(got["bias_partials"]).all(), (rows, H, form)
            else:
                with pytest.raises(_native.NativeError, match="code -3"):
                    ops.gru_gates_backward(gi, gh, b_hh, h, d_out, dh, device.lengths(data), data["t"], partials)
                got = device.finish({"bias_partials": "bias_partials"}, ("gi", "gh", "b_hh", "h", "d_out", "dh"))
                assert np.isnan(got["bias_partials"]).all(), (rows, H, form)
            assert _native.launch_counts["cusrl_gru_gates_bwd_bias"] == before + 1  # (the entry point was asked either way)
    with pytest.raises(ValueError, match=rf"\[1, 32\] tensor, got \[2, 32\]"):
        ops.gru_gates_backward(*(torch.zeros(3, w, device=DEV) for w in (24, 24)), None, torch.zeros(3, 8, device=DEV), None,
                               torch.zeros(3, 8, device=DEV), None, 0, torch.zeros(2, 32, device=DEV))


@pytest.mark.parametrize("rows", G.BIAS_ROWS)
def test_bias_folding_pass_against_float64(ops, option, rows, gradient_parity):
    """Every eligible (rows, H, form) at B = 1, rows - 1, rows, rows + 1, 3 rows + 2, with and without lengths (NaN in the ended
    rows), b_hh and d_out: gradients as the plain pass; the partial rows by count, total and block ownership; guards intact."""
    option("gru_bias_rows", rows)
    cases = G.bias_cases(rows)
    assert cases
    for case in cases:
        G.exercise(case, Device(ops, offset=_scalar_offset(case) if case.form == "scalar" else None), gradient_parity)


@pytest.mark.parametrize("form,H", [("vec", 64), ("scalar", 16)])
def test_plain_and_bias_folding_backward_give_the_same_bits(ops, form, H):
    """``gru_gates_backward`` on the same operands with and without ``bias_partials``: two kernels, one backward row — ``gi``,
    ``gh`` and ``dh`` bit for bit.  B = 17 under the default 16 rows per block: one full block and a block that owns a single
    row; 16-byte lanes at H = 64, scalars at H = 16 with ``dh`` one float off alignment; lengths that end rows (NaN in what
    an ended row may not read), with and without ``b_hh`` and ``d_out``."""
    from cusrl_amd import _native

    B, entries = 17, ("cusrl_gru_gates_bwd", "cusrl_gru_gates_bwd_bias")
    offset = "dh" if form == "scalar" else None
    for b_hh in (True, False):
        for d_out in (True, False):
            plain = G.Case(f"gru/same_bits_{form}_b{int(b_hh)}d{int(d_out)}/B{B}H{H}", "gru", B, H, lengths="mixed", garbage=True,
                           b_hh=b_hh, d_out=d_out, form=form)
            operands = G.backward_operands(G.inputs(plain))
            before = [_native.launch_counts.get(name, 0) for name in entries]
            alone = Device(ops, offset).backward(plain, operands)
            folded = Device(ops, offset).backward(dataclasses.replace(plain, rows=16), operands)
            assert [_native.launch_counts.get(name, 0) for name in entries] == [count + 1 for count in before]
            for name in ("gi", "gh", "dh"):
                assert G.same_bits(alone[name], folded[name]), (plain.name, name)


@pytest.mark.parametrize("rows,H", [(32, 32), (8, 128), (4, 256)])
def test_bias_gradients_through_the_layer(ops, option, rows, H, gradient_parity):
    """``_Gru(6, H, 1)`` over a batch with lengths, the bias-folding pass in geometries the default option never takes (H = 32
    needs 32 rows per block): d bias_ih / d bias_hh against float64 torch.nn.GRU over the PackedSequence of the same batch."""
    from cusrl_amd import _native
    from cusrl_amd.nn.rnn import _Gru

    option("gru_bias_rows", rows)
    L, B = 3, 37
    torch.manual_seed(rows * 1000 + H)
    plain = torch.nn.GRU(6, H, 1).double()
    fused = _Gru(6, H, 1).to(DEV)
    fused.load_state_dict({k: v.float() for k, v in plain.state_dict().items()})
    plain.load_state_dict({k: v.double() for k, v in fused.state_dict().items()})  # (the float32 values, exactly)
    lengths = torch.randint(1, L + 1, (B,))
    lengths[0] = L
    x, h0 = torch.randn(L, B, 6), torch.randn(B, H) * 0.3
    w_out, w_last = torch.randn(L, B, H), torch.randn(B, H)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x.double(), lengths, enforce_sorted=False)
    packed_out, want_last = plain(packed, h0.double()[None])
    want_out, _ = torch.nn.utils.rnn.pad_packed_sequence(packed_out, total_length=L)
    ((want_out * w_out.double()).sum() + (want_last[0] * w_last.double()).sum()).backward()
    before = _native.launch_counts.get("cusrl_gru_gates_bwd_bias", 0)
    out, last = fused(x.to(DEV), h0.to(DEV), lengths=lengths.to(DEV))
    ((out * w_out.to(DEV)).sum() + (last * w_last.to(DEV)).sum()).backward()
    assert _native.launch_counts.get("cusrl_gru_gates_bwd_bias", 0) - before == L
    for name in ("bias_ih_l0", "bias_hh_l0"):
        gradient_parity(f"gru_gates[layer rows{rows} H{H}:d_{name}]", getattr(fused, name).grad.cpu().numpy(),
                        getattr(plain, name).grad.numpy(), 1e-5)
