"""LatentODE backbone (reference models/LatentODE.py over lib/latent_ode_components: create_LatentODE_model, LatentODE.get_reconstruction,
Encoder_z0_ODE_RNN / Encoder_z0_RNN, GRU_unit, DiffeqSolver, ODEFunc, Decoder): an ODE-RNN walks the observed points backwards in time
(an ODE step between points, a gated update at each), transform_z0 turns its last state into the mean and deviation of z0, and the
generative ODE carries one draw of z0 over the forecast times, a Linear decoding every state.  Same class name, constructor, every
`ode_*` option with the reference's default, forecasting() signature, state_dict keys and initial values.  Self-contained: nothing of
lib/latent_ode_components is imported and neither is torchdiffeq -- the reference's DiffeqSolver hard-codes `method="rk4"`, which is one
step of the 3/8-rule RK4 per interval of the grid, written here (`rk4_step`).

Kept from the reference: the first encoder interval runs from t[-1] + 0.01; minimum_step = (t[-1] - t[0]) / 50; below it one Euler step,
else max(2, int(gap / minimum_step)) grid points; L == 1 is a GRU update from zeros with no ODE step; the update is masked by "any
feature observed at this point"; both abs() on the deviation; z0 sits at tp_to_predict[0], so the first forecast row is decoder(z0); z0
is drawn as mu + eps sigma in train and eval alike; the ValueError on a tp_to_predict that is not strictly increasing.  Dropped: the
reference's NaN asserts and prints (a host sync each).  ode_poisson / ode_classif / ode_linear_classif raise NotImplementedError (the
reference's own forecasting() has no use for what they add).

The step plan -- per observed point, Euler or the number of RK4 steps, and the step length -- is computed on the device with the
reference's float32 operations in the reference's order (`step_plan`), so it is the reference's decision bit for bit.  With the ODE-RNN
encoder, rec_layers == gen_layers == 1, n_traj_samples == 1, fp32 tensors on the GPU, no gradient wanted for the data and
immtsf_latent_ode_supported taking the widths, forecasting() is ONE HIP launch forward and TWO backward (immtsf.ops.latent_ode,
csrc/latent_ode.hip) whenever config.latentode_fused is on: the kernel reads the plan from device memory, eps is one torch.randn launch,
nothing syncs with the host (but the check of tp_to_predict, which is skipped while a graph is being captured).  `fused_calls` counts
those calls.  The kernel takes at most 256 RK4 steps per interval (the reference's plan asks for more only where the observed span is
under 0.02, through the 0.01 lead-in); the plan handed to it is clamped there.  Anything else -- and IMMTSF_LATENTODE_FUSED=0 -- runs
the composed path: the reference's loop on torch ops, which copies the plan to the host once per call (the reference syncs at every
time point) and covers every option the reference runs (any rec_layers / gen_layers / units, ode_z0_encoder='rnn', n_traj_samples > 1).

`eps_override`: None (draw), or a (n_traj_samples, B, latents) tensor used in place of the draw -- for tests against recorded noise."""
import torch
import torch.nn as nn

from immtsf import _lib, config
from immtsf.ops import latent_ode, latent_ode_supported
from immtsf.dropin import fp32_entry as _fp32_entry

MAX_FUSED_STEPS = 256      # LO_MAX_SUB of csrc/latent_ode.hip


def init_network_weights(net, std=0.1):
    for m in net.modules():
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0, std=std)
            nn.init.constant_(m.bias, val=0)


def create_net(n_inputs, n_outputs, n_layers=1, n_units=100, nonlinear=nn.Tanh):
    layers = [nn.Linear(n_inputs, n_units)]
    for _ in range(n_layers):
        layers += [nonlinear(), nn.Linear(n_units, n_units)]
    layers += [nonlinear(), nn.Linear(n_units, n_outputs)]
    return nn.Sequential(*layers)


def rk4_step(func, y, dt):
    """one step of the 3/8-rule RK4 on an autonomous function: what torchdiffeq's fixed-grid "rk4" does per interval"""
    k1 = func(y)
    k2 = func(y + dt * k1 / 3)
    k3 = func(y + dt * (k2 - k1 / 3))
    k4 = func(y + dt * (k1 - k2 + k3))
    return y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def step_plan(tp):
    """tp (L,) float32 -> (euler (L,) bool, nsub (L,) int32, gap (L,) = t_i - prev_t) for the reversed walk over the observed points:
    the reference's `(prev_t - t_i) < minimum_step` and `max(2, ((prev_t - t_i) / minimum_step).int())`, vectorised over the time axis
    with the same float32 operations in the same order; prev_t of the last point is t[-1] + 0.01.  No host sync."""
    prev = torch.cat((tp[1:], (tp[-1] + 0.01).reshape(1)))
    minimum_step = (tp[-1] - tp[0]) / 50
    gap = prev - tp
    euler = gap < minimum_step
    nsub = torch.clamp((gap / minimum_step).int(), min=2)
    return euler, nsub, tp - prev


class ODEFunc(nn.Module):
    def __init__(self, ode_func_net):
        super().__init__()
        init_network_weights(ode_func_net)
        self.gradient_net = ode_func_net

    def forward(self, y):
        return self.gradient_net(y)


class DiffeqSolver(nn.Module):
    def __init__(self, ode_func):
        super().__init__()
        self.ode_func = ode_func

    def forward(self, first_point, time_steps):
        """first_point (n, B, D), time_steps (T,) -> (n, B, T, D): one RK4 step per interval"""
        ys, y = [first_point], first_point
        for j in range(1, time_steps.shape[0]):
            y = rk4_step(self.ode_func, y, time_steps[j] - time_steps[j - 1])
            ys.append(y)
        return torch.stack(ys, 2)


class GRU_unit(nn.Module):
    def __init__(self, latent_dim, input_dim, n_units=100):
        super().__init__()
        self.update_gate = nn.Sequential(nn.Linear(latent_dim * 2 + input_dim, n_units), nn.Tanh(), nn.Linear(n_units, latent_dim), nn.Sigmoid())
        init_network_weights(self.update_gate)
        self.reset_gate = nn.Sequential(nn.Linear(latent_dim * 2 + input_dim, n_units), nn.Tanh(), nn.Linear(n_units, latent_dim), nn.Sigmoid())
        init_network_weights(self.reset_gate)
        self.new_state_net = nn.Sequential(nn.Linear(latent_dim * 2 + input_dim, n_units), nn.Tanh(), nn.Linear(n_units, latent_dim * 2))
        init_network_weights(self.new_state_net)

    def forward(self, y_mean, y_std, x):
        y_concat = torch.cat([y_mean, y_std, x], -1)
        update_gate = self.update_gate(y_concat)
        reset_gate = self.reset_gate(y_concat)
        new_state, new_state_std = self.new_state_net(torch.cat([y_mean * reset_gate, y_std * reset_gate, x], -1)).chunk(2, -1)
        new_state_std = new_state_std.abs()
        new_y = (1 - update_gate) * new_state + update_gate * y_mean
        new_y_std = (1 - update_gate) * new_state_std + update_gate * y_std
        mask = (torch.sum(x[..., x.size(-1) // 2:], -1, keepdim=True) > 0).float()      # any feature observed at this point
        new_y = mask * new_y + (1 - mask) * y_mean
        new_y_std = mask * new_y_std + (1 - mask) * y_std
        return new_y, new_y_std.abs()


class Encoder_z0_RNN(nn.Module):
    def __init__(self, latent_dim, input_dim, lstm_output_size=20):
        super().__init__()
        self.hiddens_to_z0 = nn.Sequential(nn.Linear(lstm_output_size, 50), nn.Tanh(), nn.Linear(50, latent_dim * 2))
        init_network_weights(self.hiddens_to_z0)
        self.gru_rnn = nn.GRU(input_dim + 1, lstm_output_size)

    def forward(self, data, time_steps):
        n_traj = data.size(0)
        data = data.permute(1, 0, 2).flip(0)
        delta_t = (time_steps[1:] - time_steps[:-1]).flip(0)
        delta_t = torch.cat((delta_t, torch.zeros(1, device=data.device)))
        data = torch.cat((delta_t.unsqueeze(1).repeat((1, n_traj)).unsqueeze(-1), data), -1)
        outputs, _ = self.gru_rnn(data)
        mean, std = self.hiddens_to_z0(outputs[-1]).chunk(2, -1)
        return mean.unsqueeze(0), std.abs().unsqueeze(0)


class Encoder_z0_ODE_RNN(nn.Module):
    def __init__(self, latent_dim, input_dim, z0_diffeq_solver, z0_dim, n_gru_units):
        super().__init__()
        self.GRU_update = GRU_unit(latent_dim, input_dim, n_units=n_gru_units)
        self.z0_diffeq_solver = z0_diffeq_solver
        self.latent_dim = latent_dim
        self.transform_z0 = nn.Sequential(nn.Linear(latent_dim * 2, 100), nn.Tanh(), nn.Linear(100, z0_dim * 2))
        init_network_weights(self.transform_z0)

    def forward(self, data, time_steps):
        """the composed walk: the plan comes to the host in one copy"""
        n_traj, L = data.size(0), time_steps.shape[0]
        y = torch.zeros((1, n_traj, self.latent_dim), device=data.device)
        std = torch.zeros((1, n_traj, self.latent_dim), device=data.device)
        if L == 1:
            y, std = self.GRU_update(y, std, data[:, 0, :].unsqueeze(0))
        else:
            func = self.z0_diffeq_solver.ode_func
            euler, nsub, gap = step_plan(time_steps)
            plan = torch.stack((euler.int(), nsub)).cpu().tolist()      # the one sync of a composed forward
            for i in reversed(range(L)):
                if plan[0][i]:
                    y = y + func(y) * gap[i]
                else:
                    n = plan[1][i]
                    for _ in range(n - 1):
                        y = rk4_step(func, y, gap[i] / (n - 1))
                y, std = self.GRU_update(y, std, data[:, i, :].unsqueeze(0))
        mean_z0, std_z0 = self.transform_z0(torch.cat((y, std), -1)).chunk(2, -1)
        return mean_z0, std_z0.abs()


class Decoder(nn.Module):
    def __init__(self, latent_dim, input_dim):
        super().__init__()
        decoder = nn.Sequential(nn.Linear(latent_dim, input_dim))
        init_network_weights(decoder)
        self.decoder = decoder

    def forward(self, data):
        return self.decoder(data)


class LatentODECore(nn.Module):
    """the reference's lib.latent_ode_components.latent_ode.LatentODE as create_LatentODE_model builds it (same order of draws)"""

    def __init__(self, args, input_dim):
        super().__init__()
        for name in ("poisson", "classif", "linear_classif"):
            if getattr(args, name):
                raise NotImplementedError(f"LatentODE: ode_{name} is not implemented (forecasting() has no use for it)")
        gen_ode_func = ODEFunc(create_net(args.latents, args.latents, n_layers=args.gen_layers, n_units=args.units))
        enc_input_dim = int(input_dim) * 2
        if args.z0_encoder == "odernn":
            rec_ode_func = ODEFunc(create_net(args.rec_dims, args.rec_dims, n_layers=args.rec_layers, n_units=args.units))
            encoder_z0 = Encoder_z0_ODE_RNN(args.rec_dims, enc_input_dim, DiffeqSolver(rec_ode_func), z0_dim=args.latents,
                                            n_gru_units=args.gru_units)
        elif args.z0_encoder == "rnn":
            encoder_z0 = Encoder_z0_RNN(args.latents, enc_input_dim, lstm_output_size=args.rec_dims)
        else:
            raise Exception("Unknown encoder for Latent ODE model: " + args.z0_encoder)
        decoder = Decoder(args.latents, input_dim)
        self.encoder_z0 = encoder_z0
        self.diffeq_solver = DiffeqSolver(gen_ode_func)
        self.decoder = decoder
        self.latent_dim = args.latents


class LatentODE(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.device = args.device
        self.input_dim = args.C
        self.obsrv_std_val = args.ode_obsrv_std if hasattr(args, "ode_obsrv_std") else 0.01
        defaults = {"ode_latents": 20, "ode_units": getattr(args, "ode_units", 32), "ode_gen_layers": getattr(args, "ode_gen_layers", 1),
                    "ode_rec_dims": getattr(args, "ode_rec_dims", 32), "ode_rec_layers": getattr(args, "ode_rec_layers", 1),
                    "ode_gru_units": getattr(args, "ode_gru_units", 32), "ode_poisson": False, "ode_classif": False,
                    "ode_linear_classif": False, "ode_z0_encoder": "odernn", "dataset": "custom_dataset"}

        class ArgsForODE:
            pass

        self.args_for_ode = ArgsForODE()
        self.args_for_ode.device = self.device
        self.args_for_ode.dataset = self.args.dataset
        for key_prefixed, default_value in defaults.items():
            key = key_prefixed.replace("ode_", "", 1)
            setattr(self.args_for_ode, key, getattr(self.args, key_prefixed) if hasattr(self.args, key_prefixed) else default_value)
        if self.args_for_ode.gru_units is None and hasattr(self.args, "hid_dim"):
            self.args_for_ode.gru_units = self.args.hid_dim
        elif self.args_for_ode.gru_units is None:
            self.args_for_ode.gru_units = defaults["ode_gru_units"]
        self.latent_ode_model_core = LatentODECore(self.args_for_ode, self.input_dim).to(self.device)
        self.fused_calls = 0         # forecasting() calls that took the fused HIP path (tests assert which path ran)
        self.eps_override = None     # (n_traj_samples, B, latents): used in place of the draw

    def _static_fused_ok(self):
        a = self.args_for_ode
        n_traj = self.args.ode_n_traj_samples if hasattr(self.args, "ode_n_traj_samples") else 1
        return bool(config.latentode_fused and a.z0_encoder == "odernn" and a.rec_layers == 1 and a.gen_layers == 1 and n_traj == 1 and
                    latent_ode_supported(1, 1, 1, self.input_dim, a.rec_dims, a.units, a.gru_units, a.latents))

    @property
    def immtsf_graphable(self):
        """forecasting() can be captured into a graph on the fused path only: the composed path copies the step plan to the host"""
        return self._static_fused_ok()

    def _fused_ok(self, tpp, data, tp, mask):
        a = self.args_for_ode
        B, L, C = data.shape
        if not (self._static_fused_ok() and B > 0 and C == self.input_dim and
                all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in (tpp, data, tp, mask)) and
                latent_ode_supported(B, L, tpp.shape[0], C, a.rec_dims, a.units, a.gru_units, a.latents, call=True)):
            return False
        # the module itself: a .half() / .bfloat16() model, one left on another device -> composed
        return all(q.device == data.device and q.dtype == torch.float32 for q in self.latent_ode_model_core.parameters())

    @_fp32_entry
    def forecasting(self, tp_to_predict, observed_data, observed_tp, observed_mask):
        observed_data = observed_data.to(self.device).float()
        observed_tp = observed_tp.to(self.device).float()
        observed_mask = observed_mask.to(self.device).float()
        tp_to_predict = tp_to_predict.to(self.device).float()
        if not all(t.is_cuda for t in (tp_to_predict, observed_data, observed_tp, observed_mask)):
            raise _lib.ImmtsfError("LatentODE needs tensors on the GPU (HIP); there is no CPU fallback")
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing and not torch.all(torch.diff(tp_to_predict) > 0):
            raise ValueError(f"tp_to_predict must be strictly increasing. Found: {tp_to_predict}")
        core = self.latent_ode_model_core
        n_traj_samples = self.args.ode_n_traj_samples if hasattr(self.args, "ode_n_traj_samples") else 1
        B, L, C = observed_data.shape
        eps = self.eps_override
        if eps is None:
            eps = torch.randn(n_traj_samples, B, core.latent_dim, device=observed_data.device)
        eps = eps.to(observed_data.device).float()
        if self._fused_ok(tp_to_predict, observed_data, observed_tp, observed_mask):
            self.fused_calls += 1
            if L == 1:
                steps = torch.zeros(1, dtype=torch.int32, device=observed_tp.device)
                step_len = torch.zeros(1, device=observed_tp.device)
            else:
                euler, nsub, gap = step_plan(observed_tp)
                n = torch.clamp(nsub - 1, max=MAX_FUSED_STEPS)
                steps = torch.where(euler, -1, n).int()
                step_len = torch.where(euler, gap, gap / n)
            # a net no step runs through has no gradient in the reference (None, not zeros): L == 1 skips the encoder's ODE, Lp == 1 the
            # generative one
            idle = (("encoder_z0.z0_diffeq_solver.",) if L == 1 else ()) + (("diffeq_solver.",) if tp_to_predict.shape[0] == 1 else ())
            flat = torch.cat([(p.detach() if name.startswith(idle) else p).reshape(-1) for name, p in core.named_parameters()])
            a = self.args_for_ode
            return latent_ode(observed_data, observed_mask, steps, step_len, tp_to_predict, flat, eps[0],
                              (a.rec_dims, a.units, a.gru_units, a.latents))
        first_point_mu, first_point_std = core.encoder_z0(torch.cat((observed_data, observed_mask), -1), observed_tp)
        means_z0 = first_point_mu.repeat(n_traj_samples, 1, 1)
        sigma_z0 = first_point_std.repeat(n_traj_samples, 1, 1)
        first_point_enc = eps * sigma_z0 + means_z0
        pred_x = core.decoder(core.diffeq_solver(first_point_enc, tp_to_predict))
        return pred_x.squeeze(0) if n_traj_samples == 1 else pred_x.mean(dim=0)


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
