"""Networks of the net agents (reference: rl_6_nimmt/utils/nets.py:100-144).

`MultiHeadedMLP(input, hidden_sizes, head_sizes, activation, head_activations)`
with the reference's module layout (`latent_net.<i>`, `head_nets.<h>.0`), and
`DuellingDQNNet(input, hidden_sizes, out_size, activation)`, which holds one as
`mlp` with the heads (V: 1, A: out_size) and returns [V + (A - mean A)]
(`mlp.latent_net.*`, `mlp.head_nets.0.0.*` = V, `mlp.head_nets.1.0.*` = A):
state_dicts are interchangeable with the reference's.

`NoisyFactorizedLinear(in, out, sigma_init)` (reference utils/nets.py:36-63) is
the factorised-Gaussian NoisyNet layer of the noisy DQN agents: nn.Linear plus
`sigma_weight [out, in]` and `sigma_bias [out]` (both sigma_init / sqrt(in)) and
the buffers `epsilon_input [1, in]`, `epsilon_output [out, 1]`, redrawn with
torch.randn on every forward (input first), in eval() mode too.  Both nets
take `linear=NoisyFactorizedLinear` and hand `init_sigma` to every layer.  The
reference's unfactorised `NoisyLinear` is not built (no agent uses it); any
other `linear=` raises.
"""
import functools
import math

import torch
from torch import nn
from torch.nn import functional as F


def signed_sqrt(x):
    """f(x) = sign(x) * sqrt|x|, the factorised noise's shaping"""
    return torch.sign(x) * torch.sqrt(torch.abs(x))


class NoisyFactorizedLinear(nn.Linear):
    """y = x (W + S o (f(e_out) f(e_in)^T))^T + b + s_b o f(e_out), one fresh (e_in, e_out) per forward"""

    def __init__(self, in_features, out_features, sigma_init=0.4, bias=True):
        super().__init__(in_features, out_features, bias=bias)
        sigma = sigma_init / math.sqrt(in_features)
        self.sigma_weight = nn.Parameter(torch.full((out_features, in_features), sigma))
        self.register_buffer("epsilon_input", torch.zeros(1, in_features))
        self.register_buffer("epsilon_output", torch.zeros(out_features, 1))
        if bias:
            self.sigma_bias = nn.Parameter(torch.full((out_features,), sigma))

    def forward(self, inputs):
        torch.randn(self.epsilon_input.size(), out=self.epsilon_input)
        torch.randn(self.epsilon_output.size(), out=self.epsilon_output)
        e_in, e_out = signed_sqrt(self.epsilon_input), signed_sqrt(self.epsilon_output)
        weight = self.weight + self.sigma_weight * (e_in * e_out)
        bias = None if self.bias is None else self.bias + self.sigma_bias * e_out.view(-1)
        return F.linear(inputs, weight, bias)


class MultiHeadedMLP(nn.Module):
    def __init__(self, input_size, hidden_sizes, head_sizes, activation, head_activations, linear=nn.Linear,
                 init_sigma=1.0):
        super().__init__()
        if linear is NoisyFactorizedLinear:
            linear = functools.partial(linear, sigma_init=init_sigma)
        elif linear is not nn.Linear:
            raise NotImplementedError("only nn.Linear and NoisyFactorizedLinear layers are built")
        layers, width = [], input_size
        for h in hidden_sizes:
            layers += [linear(width, h), activation]
            width = h
        self.latent_net = nn.Sequential(*layers)
        self.head_nets = nn.ModuleList()
        for size, act in zip(head_sizes, head_activations):
            head = [linear(width, size)] + ([act] if act is not None else [])
            self.head_nets.append(nn.Sequential(*head))

    def forward(self, inputs):
        latent = self.latent_net(inputs)
        return [head(latent) for head in self.head_nets]


class DuellingDQNNet(nn.Module):
    def __init__(self, input_size, hidden_sizes, out_size, activation, linear=nn.Linear, init_sigma=1.0):
        super().__init__()
        self.mlp = MultiHeadedMLP(input_size, hidden_sizes, (1, out_size), activation, (None, None), linear=linear,
                                  init_sigma=init_sigma)

    def forward(self, inputs):
        V, A = self.mlp(inputs)
        return [V + (A - A.mean(keepdim=True, dim=-1))]
