"""NeuralFlow backbone (reference models/NeuralFlow.py over lib/neural_flow_components: create_LatentODE_model at model = 'flow',
LatentODE.get_reconstruction, Encoder_z0_ODE_RNN with its LSTM cell, SolverWrapper, models/flow.py's CouplingFlow, Decoder): the encoder
walks the observed points backwards in time (a flow step over the gap between points, an LSTM cell update at each), transform_z0 turns
its last hidden state into the mean and, through softplus, the deviation of z0, and the generative flow carries one draw of z0 to every
forecast time in closed form, a Linear decoding every state.  Same class name, constructor reads (input_len, pred_len, enc_in, device
and every `nf_*` option with the reference's default), forecasting() signature, state_dict keys and initial values.  Self-contained:
nothing of lib/neural_flow_components, of lib.utils or of `stribor` is imported.

`stribor` supplies the reference's coupling layer (ContinuousAffineCoupling, Flow, net.MLP, net.TimeLinear, net.TimeTanh) and is not
installed where this was written, so the layer is WRITTEN OUT here from the published definition (Bilos et al., "Neural Flows", 2021,
the coupling flow) as stribor 0.1.0 is remembered to implement it, and COULD NOT BE CHECKED AGAINST THE PACKAGE: for layer i with
m = ordered_{i % 2} (m_j = 1 for j < dim // 2 at even i, the complement at odd i; all zero at dim == 1),
    (s, b) = latent_net(cat(x m, t)).chunk(2, -1),  (phi_s, phi_b) = time_net(t).chunk(2, -1),
    y = x exp(s phi_s) + b phi_b,  out = y (1 - m) + x m,
latent_net = MLP(dim + 1 -> hidden_dims -> 2 dim) with Tanh between its Linears, time_net = TimeLinear (scale t, `scale` (1, 2 dim)) or
TimeTanh (tanh(scale t)).  Equally from memory: the part of the state_dict keys that stribor names (`flow.transforms.N`,
`latent_net.net.N`, `time_net.scale`) and the initial value of `scale` (xavier_uniform_ on (1, 2 dim)); a checkpoint interchanges with
the reference's only as far as those hold.  The goldens (tests/golden/make_golden_neuralflow.py) run the reference's own code around a
stand-in of the same definition.

Kept from the reference: the first encoder interval runs from t[:, -1] + 0.01; the flow's time argument is t_i - prev_t (negative); the
flow step runs at padded and unobserved points too; the LSTM update is kept where any feature of the point is observed; `time_steps[:,
i - 1]` wraps around at i = 0 and the value is never used; z0 is drawn as mu + eps sigma in train and eval alike, one sample; every
window has its own observed and forecast times; ValueError('Unknown flow transformation') for a flow_model the reference rejects.
Dropped: the reference's NaN asserts, utils.check_mask and the `first_point_std < 0` assert (a host sync each).  nf_flow_model='resnet'
and any nf_time_net but TimeLinear / TimeTanh raise NotImplementedError: they need stribor's spectral-norm ResNet and Fourier nets,
which are not restated.  The options of the reference's ODE branch (nf_solver, nf_odenet, ...) are read and unused, as there
(create_LatentODE_model is called with model = 'flow').

With the TimeLinear time net, fp32 tensors on the GPU, no gradient wanted for the data and immtsf_neural_flow_supported taking the
widths, forecasting() is TWO HIP launches forward and THREE backward (immtsf.ops.neural_flow, csrc/neural_flow.hip) whenever
config.neuralflow_fused is on; eps is one torch.randn launch, every window's times are read from device memory, nothing syncs with the
host.  The TimeTanh time net takes the same launches (the kernels' TimeTanh instance) under the same conditions once
config.neuralflow_tanh_fused is on as well (IMMTSF_NEURALFLOW_TANH_FUSED=1; off by default, see immtsf/config.py).  `fused_calls`
counts the calls of either kind.  Anything else -- and IMMTSF_NEURALFLOW_FUSED=0 -- runs the composed path: the reference's
loop on torch ops, which covers every option the reference's forecasting() reaches with the coupling flow (any nf_flow_layers,
nf_hidden_layers, nf_hidden_dim, nf_rec_dims, nf_latents, TimeTanh) and does not sync either.

`eps_override`: None (draw), or a (1, B, latents) tensor used in place of the draw -- for tests against recorded noise."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from immtsf import _lib, config
from immtsf.ops import neural_flow, neural_flow_supported
from immtsf.dropin import fp32_entry as _fp32_entry

TIME_NETS = ("TimeLinear", "TimeTanh")


def init_network_weights(net, std=0.1):
    for m in net.modules():
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0, std=std)
            nn.init.constant_(m.bias, val=0)


class MLP(nn.Module):
    """Linear layers in_dim -> hidden_dims... -> out_dim with Tanh between them and none behind the last (`net`, a Sequential)"""

    def __init__(self, in_dim, hidden_dims, out_dim):
        super().__init__()
        dims = [in_dim] + list(hidden_dims) + [out_dim]
        layers = []
        for a, b in zip(dims[:-1], dims[1:]):
            layers += [nn.Linear(a, b), nn.Tanh()]
        self.net = nn.Sequential(*layers[:-1])

    def forward(self, x):
        return self.net(x)


class TimeLinear(nn.Module):
    def __init__(self, out_dim, hidden_dim=None):
        super().__init__()
        self.scale = nn.Parameter(torch.empty(1, out_dim))
        nn.init.xavier_uniform_(self.scale)

    def forward(self, t):
        return self.scale * t


class TimeTanh(TimeLinear):
    def forward(self, t):
        return torch.tanh(self.scale * t)


def coupling_mask(dim, layer):
    """ordered_{layer % 2} as a (dim,) float tensor; 'none' (all zeros) at dim == 1"""
    m = torch.zeros(dim)
    if dim > 1:
        m[:dim // 2] = 1
        if layer % 2:
            m = 1 - m
    return m


class ContinuousAffineCoupling(nn.Module):
    def __init__(self, latent_net, time_net, dim, layer):
        super().__init__()
        self.latent_net = latent_net
        self.time_net = time_net
        self.register_buffer("mask", coupling_mask(dim, layer), persistent=False)

    def forward(self, x, t):
        m = self.mask.to(x.dtype)
        s, b = self.latent_net(torch.cat((x * m, t), -1)).chunk(2, -1)
        phi_s, phi_b = self.time_net(t).chunk(2, -1)
        y = x * torch.exp(s * phi_s) + b * phi_b
        return y * (1 - m) + x * m


class Flow(nn.Module):
    def __init__(self, transforms):
        super().__init__()
        self.transforms = nn.ModuleList(transforms)

    def forward(self, x, t):
        for f in self.transforms:
            x = f(x, t)
        return x


class CouplingFlow(nn.Module):
    def __init__(self, dim, n_layers, hidden_dims, time_net, time_hidden_dim=None):
        super().__init__()
        if time_net not in TIME_NETS:
            raise NotImplementedError(f"NeuralFlow: nf_time_net={time_net!r} is not implemented (TimeLinear and TimeTanh are; the others "
                                      "need stribor's nets)")
        make_time = TimeLinear if time_net == "TimeLinear" else TimeTanh
        self.flow = Flow([ContinuousAffineCoupling(MLP(dim + 1, hidden_dims, 2 * dim), make_time(2 * dim, hidden_dim=time_hidden_dim), dim, i)
                          for i in range(n_layers)])

    def forward(self, x, t):
        """x (..., dim), t (..., 1) -> the state at t (..., dim)"""
        return self.flow(x, t)


class SolverWrapper(nn.Module):
    def __init__(self, solver):
        super().__init__()
        self.solver = solver

    def forward(self, x, t):
        return self.solver(x, t)


class Encoder_z0_ODE_RNN(nn.Module):
    def __init__(self, latent_dim, input_dim, z0_diffeq_solver, z0_dim):
        super().__init__()
        self.lstm = nn.LSTMCell(input_dim, latent_dim)
        self.z0_diffeq_solver = z0_diffeq_solver
        self.latent_dim = latent_dim
        self.transform_z0 = nn.Sequential(nn.Linear(latent_dim, 100), nn.Tanh(), nn.Linear(100, z0_dim * 2))
        init_network_weights(self.transform_z0)

    def forward(self, data, time_steps):
        """data (B, L, 2C), time_steps (B, L) -> (mu, sigma), each (B, z0_dim): the composed walk, last point first"""
        B, L, _ = data.shape
        prev_t, t_i = time_steps[:, -1] + 0.01, time_steps[:, -1]
        h = torch.zeros(B, self.latent_dim, device=data.device, dtype=data.dtype)
        c = torch.zeros_like(h)
        for i in reversed(range(L)):
            h = self.z0_diffeq_solver(h, (t_i - prev_t).unsqueeze(1))
            xi = data[:, i, :]
            h_, c_ = self.lstm(xi, (h, c))
            mask = (torch.sum(xi[:, xi.size(-1) // 2:], -1, keepdim=True) > 0).to(h.dtype)      # any feature observed at this point
            h = mask * h_ + (1 - mask) * h
            c = mask * c_ + (1 - mask) * c
            prev_t, t_i = time_steps[:, i], time_steps[:, i - 1]      # i = 0 wraps around; the value is never used
        mean_z0, std_z0 = self.transform_z0(h).chunk(2, dim=-1)
        return mean_z0, F.softplus(std_z0)


class Decoder(nn.Module):
    def __init__(self, latent_dim, input_dim):
        super().__init__()
        decoder = nn.Sequential(nn.Linear(latent_dim, input_dim))
        init_network_weights(decoder)
        self.decoder = decoder

    def forward(self, data):
        return self.decoder(data)


class NeuralFlowCore(nn.Module):
    """the reference's lib.neural_flow_components LatentODE as create_LatentODE_model builds it at model = 'flow' (same order of draws)"""

    def __init__(self, args, input_dim):
        super().__init__()
        hidden_dims = [args.hidden_dim] * args.hidden_layers
        if args.flow_model == "coupling":
            flow = CouplingFlow
        elif args.flow_model == "resnet":
            raise NotImplementedError("NeuralFlow: nf_flow_model='resnet' is not implemented (it needs stribor's spectral-norm ResNet)")
        else:
            raise ValueError("Unknown flow transformation")
        z0_diffeq_solver = SolverWrapper(flow(args.rec_dims, args.flow_layers, hidden_dims, args.time_net, args.time_hidden_dim))
        diffeq_solver = SolverWrapper(flow(args.latents, args.flow_layers, hidden_dims, args.time_net, args.time_hidden_dim))
        self.encoder_z0 = Encoder_z0_ODE_RNN(args.rec_dims, int(input_dim) * 2, z0_diffeq_solver, z0_dim=args.latents)
        self.diffeq_solver = diffeq_solver
        self.decoder = Decoder(args.latents, input_dim)
        self.latent_dim = args.latents


class NeuralFlow(nn.Module):
    def __init__(self, configs):
        super().__init__()
        self.input_len = configs.input_len
        self.pred_len = configs.pred_len
        self.enc_in = configs.enc_in
        self.device = configs.device

        class NF_Args_Internal:
            def __init__(self):
                self.model = "flow"
                self.experiment = "latent_ode"
                self.latents = getattr(configs, "nf_latents", 20)
                self.rec_dims = getattr(configs, "nf_rec_dims", 40)
                self.gru_units = getattr(configs, "nf_gru_units", 32)
                self.hidden_layers = getattr(configs, "nf_hidden_layers", 3)
                self.hidden_dim = getattr(configs, "nf_hidden_dim", 32)
                self.flow_model = getattr(configs, "nf_flow_model", "coupling")
                self.flow_layers = getattr(configs, "nf_flow_layers", 2)
                self.time_net = getattr(configs, "nf_time_net", "TimeLinear")
                self.time_hidden_dim = getattr(configs, "nf_time_hidden_dim", 8)
                self.solver = getattr(configs, "nf_solver", "dopri5")
                self.solver_step = getattr(configs, "nf_solver_step", 0.05)
                self.atol = getattr(configs, "nf_atol", 1e-4)
                self.rtol = getattr(configs, "nf_rtol", 1e-3)
                self.odenet = getattr(configs, "nf_odenet", "concat")
                self.activation = getattr(configs, "nf_activation", "Tanh")
                self.final_activation = getattr(configs, "nf_final_activation", "Identity")
                self.input_dim = configs.enc_in
                self.classify = 0
                self.extrap = getattr(configs, "nf_extrap", 0)
                self.device = configs.device
                self.weight_decay = getattr(configs, "nf_weight_decay", 0.0001)
                self.quantization = getattr(configs, "nf_quantization", 0.0)
                self.max_t = getattr(configs, "nf_max_t", 5.)
                self.mixing = getattr(configs, "nf_mixing", 0.0001)
                self.gob_prep_hidden = getattr(configs, "nf_gob_prep_hidden", 10)
                self.gob_cov_hidden = getattr(configs, "nf_gob_cov_hidden", 50)
                self.gob_p_hidden = getattr(configs, "nf_gob_p_hidden", 25)
                self.invertible = getattr(configs, "nf_invertible", 1)
                self.components = getattr(configs, "nf_components", 8)
                self.decoder = getattr(configs, "nf_decoder_type", "continuous")
                self.rnn = getattr(configs, "nf_rnn", "gru")
                self.marks = getattr(configs, "nf_marks", 0)
                self.density_model = getattr(configs, "nf_density_model", "independent")

        self.nf_args = NF_Args_Internal()
        self.obsrv_std_val = getattr(configs, "nf_obsrv_std", 0.01)
        self.n_classes = 0
        self.nf_model_core = NeuralFlowCore(self.nf_args, self.enc_in).to(self.device)
        self.fused_calls = 0         # forecasting() calls that took the fused HIP path (tests assert which path ran)
        self.eps_override = None     # (1, B, latents): used in place of the draw

    def _widths(self):
        a = self.nf_args
        return (a.rec_dims, a.latents, a.hidden_dim, a.hidden_layers, a.flow_layers)

    def _time_net_fused(self):
        """the knobs: TimeLinear under config.neuralflow_fused, TimeTanh under config.neuralflow_tanh_fused as well"""
        tn = self.nf_args.time_net
        return bool(config.neuralflow_fused and (tn == "TimeLinear" or (tn == "TimeTanh" and config.neuralflow_tanh_fused)))

    def _static_fused_ok(self):
        return self._time_net_fused() and neural_flow_supported(1, 1, 1, self.enc_in, *self._widths(), time_net=self.nf_args.time_net)

    @property
    def immtsf_graphable(self):
        """forecasting() has no host sync on either path; what a captured graph replays follows the knob at capture"""
        return True

    def _fused_ok(self, tpp, data, tp, mask):
        B, L, C = data.shape
        if not (self._static_fused_ok() and B > 0 and C == self.enc_in and tpp.dim() == 2 and tp.dim() == 2 and
                all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in (tpp, data, tp, mask)) and
                neural_flow_supported(B, L, tpp.shape[1], C, *self._widths(), call=True, time_net=self.nf_args.time_net)):
            return False
        # the module itself: a .half() / .bfloat16() model, one left on another device -> composed
        return all(q.device == data.device and q.dtype == torch.float32 for q in self.nf_model_core.parameters())

    @_fp32_entry
    def forecasting(self, tp_to_predict, observed_data, observed_tp, observed_mask):
        """tp_to_predict (B, Lp), observed_data (B, L, C), observed_tp (B, L), observed_mask (B, L, C) -> (B, Lp, C)"""
        observed_data = observed_data.to(self.device).float()
        observed_tp = observed_tp.to(self.device).float()
        observed_mask = observed_mask.to(self.device).float()
        tp_to_predict = tp_to_predict.to(self.device).float()
        if not all(t.is_cuda for t in (tp_to_predict, observed_data, observed_tp, observed_mask)):
            raise _lib.ImmtsfError("NeuralFlow needs tensors on the GPU (HIP); there is no CPU fallback")
        core = self.nf_model_core
        B, L, C = observed_data.shape
        eps = self.eps_override
        if eps is None:
            eps = torch.randn(1, B, core.latent_dim, device=observed_data.device)
        eps = eps.to(observed_data.device).float().reshape(B, core.latent_dim)
        if self._fused_ok(tp_to_predict, observed_data, observed_tp, observed_mask):
            self.fused_calls += 1
            flat = torch.cat([p.reshape(-1) for p in core.parameters()])
            return neural_flow(observed_data, observed_mask, observed_tp, tp_to_predict, flat, eps, self._widths(), self.nf_args.time_net)
        mu, sigma = core.encoder_z0(torch.cat((observed_data, observed_mask), -1), observed_tp)
        z0 = eps * sigma + mu
        Lp = tp_to_predict.shape[1]
        sol_y = core.diffeq_solver(z0.unsqueeze(1).expand(B, Lp, core.latent_dim), tp_to_predict.unsqueeze(-1))
        return core.decoder(sol_y)


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
