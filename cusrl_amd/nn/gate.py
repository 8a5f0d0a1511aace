"""Gate layers that merge a stream ``x`` with a branch ``y`` (counterpart of cusrl/nn/layer/gate.py:17-154): the pieces the
reference's transformer layers put around attention and feed-forward, usable by themselves in a user's ``Module``.  Same
constructors, sub-module names, bias presence, initial bias fills and ``get_gate_cls`` error text as the reference, so its state
dicts load strictly.  The linear layers are library GEMMs; everything between them is one launch per direction
(``ops.gate_combine``, DESIGN.md "Gates and GLU")."""

from __future__ import annotations

from torch import Tensor, nn

__all__ = ["Gate", "GruGate", "HighwayGate", "InputGate", "OutputGate", "PassthroughGate", "ResidualGate", "SigmoidTanhGate",
           "gate_map", "get_gate_cls"]


def _combine(kind: str, *operands, **more) -> Tensor:
    from cusrl_amd import ops

    return ops.gate_combine(kind, *operands, **more)


class Gate(nn.Module):
    def __init__(self, embed_dim: int):
        super().__init__()
        self.embed_dim = embed_dim

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        raise NotImplementedError


class PassthroughGate(Gate):
    """``y``."""

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        return y


class ResidualGate(Gate):
    """``x + y``."""

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        return x + y


class InputGate(Gate):
    """``sigmoid(W x) * x + y``."""

    def __init__(self, embed_dim: int):
        super().__init__(embed_dim)
        self.gate_linear = nn.Linear(embed_dim, embed_dim, bias=False)

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        return _combine("input", x, y, self.gate_linear(x))


class OutputGate(Gate):
    """``x + sigmoid(W x + b) * y``, ``b`` initially -1."""

    def __init__(self, embed_dim: int):
        super().__init__(embed_dim)
        self.gate_linear = nn.Linear(embed_dim, embed_dim)
        self.gate_linear.bias.data.fill_(-1.0)

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        return _combine("output", x, y, self.gate_linear(x))


class HighwayGate(Gate):
    """``g * x + (1 - g) * y`` with ``g = sigmoid(W x + b)``, ``b`` initially +1."""

    def __init__(self, embed_dim: int):
        super().__init__(embed_dim)
        self.gate_linear = nn.Linear(embed_dim, embed_dim)
        self.gate_linear.bias.data.fill_(1.0)

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        return _combine("highway", x, y, self.gate_linear(x))


class SigmoidTanhGate(Gate):
    """``x + sigmoid(W y + b) * tanh(U y)``, ``b`` initially -1."""

    def __init__(self, embed_dim: int):
        super().__init__(embed_dim)
        self.sigmoid_linear = nn.Linear(embed_dim, embed_dim)
        self.sigmoid_linear.bias.data.fill_(-1.0)
        self.tanh_linear = nn.Linear(embed_dim, embed_dim, bias=False)

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        return _combine("sigmoid_tanh", x, None, self.sigmoid_linear(y), self.tanh_linear(y))


class GruGate(Gate):
    """The GRU-style gate of "Stabilizing Transformers for Reinforcement Learning" (Parisotto et al., 2020):
    ``r = sigmoid(W_r y + U_r x)``, ``z = sigmoid(W_z y + U_z x + b)`` with ``b`` initially -2,
    ``h = tanh(W_h y + U_h (r * x))``, output ``(1 - z) * x + z * h``.  Six GEMMs and two launches: the reset product, and
    everything behind the last GEMM."""

    def __init__(self, embed_dim: int):
        super().__init__(embed_dim)
        self.r_y = nn.Linear(embed_dim, embed_dim, bias=False)
        self.r_x = nn.Linear(embed_dim, embed_dim, bias=False)
        self.z_y = nn.Linear(embed_dim, embed_dim, bias=False)
        self.z_x = nn.Linear(embed_dim, embed_dim)
        self.z_x.bias.data.fill_(-2.0)
        self.h_y = nn.Linear(embed_dim, embed_dim, bias=False)
        self.h_rx = nn.Linear(embed_dim, embed_dim, bias=False)

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        reset_x = _combine("gru_reset", x, None, self.r_y(y), p2=self.r_x(x))
        return _combine("gru_out", x, None, self.z_y(y), self.h_y(y), p2=self.z_x(x), q2=self.h_rx(reset_x))


gate_map = {
    None: PassthroughGate,
    "gru": GruGate,
    "highway": HighwayGate,
    "input": InputGate,
    "output": OutputGate,
    "residual": ResidualGate,
    "sigmoid_tanh": SigmoidTanhGate,
}


def get_gate_cls(gate_type: str | None) -> type[Gate]:
    if (gate_cls := gate_map.get(gate_type)) is None:
        available = ", ".join(repr(name) for name in gate_map.keys())
        raise ValueError(f"Unsupported gate type '{gate_type}'; available gate types: {available}")
    return gate_cls
