"""CRU backbone (reference models/CRU.py:7-97 over lib/cru_components: Physionet_USHCN, CRU_Module, CRULayer, CRUCell / RKNCell, Encoder,
SplitDiagGaussianDecoder): an encoder of three Linear -> ReLU -> LayerNorm blocks gives a latent observation and its variance per time
point, a Kalman filter with a locally linear, continuous-time transition walks the history and the horizon (update at observed points,
exp(A dt) predict in between), and the mean decoder maps the posterior means of the horizon to the C channels.  Same class name,
constructor, forecasting() signature, state_dict keys, initial values and gradient-less parameters (the variance decoder, which
forecasting() never reads).  Self-contained: nothing of lib/cru_components is imported.

The encoder and the mean decoder are rows: immtsf.ops.linear (one HIP GEMM each, ReLU fused) and immtsf.ops.layer_norm on both paths;
the encoder runs on the L history rows only (the horizon's rows are masked by the update), the decoder on the Lp horizon rows only.
The recurrence between them is ONE HIP launch (immtsf.ops.cru_scan, csrc/cru.hip) and its backward TWO whenever config.cru_fused is
on, the cell is the continuous CRUCell (neither cru_rkn nor cru_f_cru) with the single Linear + softmax coefficient net (no hidden
units, not time-sensitive), the tensors are fp32 on the GPU, immtsf_cru_supported takes the shape and neither data, mask nor times
wants a gradient; `fused_calls` counts those calls.  Anything else -- and IMMTSF_CRU_FUSED=0 -- runs the composed path: the
reference's Python loop over the time points with torch ops (torch.matrix_exp of A dt and of the Van Loan block matrix) around
immtsf.ops.linear, which covers every option the reference runs.  The fused path is fp32 in bf16 mode too.

Kept from the reference: an odd cru_lsd raises, cru_f_cru=True raises the AttributeError on `orthogonal`, a time-sensitive coefficient
net on the continuous cell fails in torch.cat.  Dropped: the per-step `print` check of the side covariance (a host sync per time
point) and the predict after the last time point, which has no reader.  The fused path never syncs with the host and is captured
into graphs (`immtsf_graphable`); the composed continuous cell inherits torch.matrix_exp's own read of a batch's norms on the host."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from immtsf import config
from immtsf.ops import cru_scan, cru_supported, layer_norm, linear
from immtsf.dropin import fp32_entry as _fp32_entry


def _variance(x, kind, soft="elup1"):
    """the five variance activations; the encoder's / decoder's fifth is elu + 1, the cell's (any other name) is softplus"""
    if kind == "exp":
        return torch.exp(x)
    if kind == "relu":
        return torch.maximum(x, torch.zeros_like(x))
    if kind == "square":
        return torch.square(x)
    if kind == "abs":
        return torch.abs(x)
    if soft == "softplus":
        return torch.log(torch.exp(x) + 1.0)
    if kind == "elup1":
        return torch.exp(x).where(x < 0.0, x + 1.0)
    raise Exception("Variance activation function unknown.")


def _variance_inverse(v, kind):
    if kind == "exp":
        return np.log(v)
    if kind == "square":
        return np.sqrt(v)
    if kind in ("relu", "abs"):
        return v
    return np.log(np.exp(v) - 1.0)


def _stack(layers, h):
    """[Linear, ReLU, LayerNorm] * k on rows: one GEMM (ReLU fused) and one LayerNorm kernel per block"""
    for i in range(0, len(layers), 3):
        h = linear(h, layers[i].weight, layers[i].bias, relu=True)
        h = layer_norm(h, layers[i + 2].weight, layers[i + 2].bias, layers[i + 2].eps)
    return h


def _blocks(sizes):
    layers = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        layers += [nn.Linear(a, b), nn.ReLU(), nn.LayerNorm(b)]
    return nn.ModuleList(layers)


def _bmv(mat, vec):
    return torch.bmm(mat, vec[..., None])[..., 0]


class RKNCell(nn.Module):
    """the discrete cell (cru_rkn): the transition matrix is I + the basis mix and is applied as it stands"""

    def __init__(self, latent_obs_dim, args, dtype=torch.float32):
        super().__init__()
        self._lod = latent_obs_dim
        self._lsd = 2 * latent_obs_dim
        self.args = args
        self._dtype = dtype
        if args.f_cru:      # the reference's CRU_Args_Internal carries no `orthogonal`: building an f-CRU fails on it, here as there
            raise AttributeError("'CRU_Args_Internal' object has no attribute 'orthogonal'")
        lod, bw = self._lod, args.bandwidth
        self._num_entries = int(lod + 2 * np.sum(np.arange(lod - bw, lod)))
        band = np.triu(np.ones([lod, lod], dtype=np.float32), -bw) * np.tril(np.ones([lod, lod], dtype=np.float32), bw)
        idx = torch.where(torch.tensor(band, dtype=torch.bool))
        self.register_buffer("_idx0", idx[0], persistent=False)
        self.register_buffer("_idx1", idx[1], persistent=False)
        self.register_buffer("_diag_idx", torch.where(idx[0] == idx[1])[0], persistent=False)
        shape = (args.num_basis, self._num_entries)
        self._tm_11_basis = nn.Parameter(torch.zeros(shape, dtype=dtype))
        tm12, tm21 = torch.zeros(shape, dtype=dtype), torch.zeros(shape, dtype=dtype)
        if args.rkn:
            tm12[:, self._diag_idx] += 0.2 * torch.ones(lod)
            tm21[:, self._diag_idx] -= 0.2 * torch.ones(lod)
        self._tm_12_basis = nn.Parameter(tm12)
        self._tm_21_basis = nn.Parameter(tm21)
        self._tm_22_basis = nn.Parameter(torch.zeros(shape, dtype=dtype))
        layers, prev = [], self._lsd + 1 if args.t_sensitive_trans_net else self._lsd
        for n in args.trans_net_hidden_units:
            layers += [nn.Linear(prev, n), getattr(nn, args.trans_net_hidden_activation)()]
            prev = n
        layers += [nn.Linear(prev, args.num_basis), nn.Softmax(dim=-1)]
        self._coefficient_net = nn.Sequential(*layers).to(dtype=dtype)
        self._log_transition_noise = nn.Parameter(torch.full((1, self._lsd), float(_variance_inverse(args.trans_covar, args.trans_var_activation)),
                                                             dtype=dtype))

    def transition_variance(self):
        return _variance(self._log_transition_noise, self.args.trans_var_activation, soft="softplus")

    def bases(self):
        return self._tm_11_basis, self._tm_12_basis, self._tm_21_basis, self._tm_22_basis

    def _unflatten(self, flat):
        tm = torch.zeros(flat.shape[0], self._lod, self._lod, device=flat.device, dtype=self._dtype)
        tm[:, self._idx0, self._idx1] = flat
        return tm

    def transition(self, post_mean, delta_t):
        x = torch.cat([post_mean, delta_t[:, None]], 1) if self.args.t_sensitive_trans_net else post_mean
        net = list(self._coefficient_net)
        for i in range(0, len(net) - 2, 2):
            x = net[i + 1](linear(x, net[i].weight, net[i].bias))
        coeff = torch.softmax(linear(x, net[-2].weight, net[-2].bias), -1)[:, :, None]
        flats = [(coeff * basis).sum(dim=1) for basis in self.bases()]
        if self.args.rkn:
            flats[0] = flats[0].index_add(1, self._diag_idx, torch.ones(flats[0].shape[0], self._lod, device=flats[0].device))
            flats[3] = flats[3].index_add(1, self._diag_idx, torch.ones(flats[3].shape[0], self._lod, device=flats[3].device))
        return [self._unflatten(f) for f in flats]

    def update(self, prior_mean, prior_cov, obs, obs_var, obs_valid):
        cu, cl, cs = prior_cov
        den = cu + obs_var
        qu, ql = cu / den, cs / den
        res = obs - prior_mean[:, :self._lod]
        mean = prior_mean + torch.cat([qu * res, ql * res], -1)
        factor = 1 - qu
        v = obs_valid[..., None]
        return mean.where(v, prior_mean), [(factor * cu).where(v, cu), (cl - ql * cs).where(v, cl), (factor * cs).where(v, cs)]

    def predict(self, post_mean, post_cov, delta_t):
        tm11, tm12, tm21, tm22 = self.transition(post_mean, delta_t)
        q = self.transition_variance()
        mu, ml = post_mean[:, :self._lod], post_mean[:, self._lod:]
        cu, cl, cs = post_cov
        nmu = _bmv(tm11, mu) + _bmv(tm12, ml)
        nml = _bmv(tm21, mu) + _bmv(tm22, ml)
        ncu = _bmv(tm11.square(), cu) + 2.0 * _bmv(tm11 * tm12, cs) + _bmv(tm12.square(), cl) + q[..., :self._lod]
        ncl = _bmv(tm21.square(), cu) + 2.0 * _bmv(tm21 * tm22, cs) + _bmv(tm22.square(), cl) + q[..., self._lod:]
        ncs = _bmv(tm21 * tm11, cu) + _bmv(tm22 * tm11, cs) + _bmv(tm21 * tm12, cs) + _bmv(tm22 * tm12, cl)
        return torch.cat([nmu, nml], dim=-1), [ncu, ncl, ncs]


class CRUCell(RKNCell):
    """the continuous cell: exp(A dt) on the mean, the Van Loan block matrix for the covariance (CRUCell.py:357-391, :437-500)"""

    def predict(self, post_mean, post_cov, delta_t):
        lod, lsd = self._lod, self._lsd
        delta_t = delta_t[:, None, None]
        tm11, tm12, tm21, tm22 = self.transition(post_mean, delta_t)
        Q = torch.diag_embed(self.transition_variance().repeat(post_mean.shape[0], 1))
        cu, cl, cs = [torch.diag_embed(x) for x in post_cov]
        Sigma = torch.cat((torch.cat((cu, cs), -1), torch.cat((cs, cl), -1)), -2)
        A = torch.cat((torch.cat((tm11, tm12), -1), torch.cat((tm21, tm22), -1)), -2)
        exp_A = torch.matrix_exp(A * delta_t)
        Bm = torch.cat((torch.cat((A, Q), -1), torch.cat((torch.zeros_like(Q), -A.transpose(-2, -1)), -1)), -2)
        M2 = torch.matrix_exp(Bm * delta_t)[:, :lsd, lsd:]
        prior = torch.matmul(torch.matmul(exp_A, Sigma) + M2, exp_A.transpose(-2, -1))
        diag = lambda x: torch.diagonal(x, dim1=-1, dim2=-2)      # noqa: E731
        return _bmv(exp_A, post_mean), [diag(prior[:, :lod, :lod]), diag(prior[:, lod:, lod:]), diag(prior[:, :lod, lod:])]


class CRULayer(nn.Module):
    def __init__(self, latent_obs_dim, args, dtype=torch.float32):
        super().__init__()
        self._lod = latent_obs_dim
        self._lsd = 2 * latent_obs_dim
        self._cell = RKNCell(latent_obs_dim, args, dtype) if args.rkn else CRUCell(latent_obs_dim, args, dtype)

    def forward(self, latent_obs, obs_vars, initial_mean, initial_cov, obs_valid, time_points):
        """the reference's loop over the T time points, without the predict after the last one -> the posterior means (B, T, lsd)"""
        prior_mean, prior_cov = initial_mean, initial_cov
        T, means = latent_obs.shape[1], []
        for i in range(T):
            post_mean, post_cov = self._cell.update(prior_mean, prior_cov, latent_obs[:, i], obs_vars[:, i], obs_valid[:, i])
            means.append(post_mean)
            if i < T - 1:
                prior_mean, prior_cov = self._cell.predict(post_mean, post_cov, time_points[:, i + 1] - time_points[:, i])
        return torch.stack(means, 1)


class TimeDistributed(nn.Module):
    """the wrapper whose `_module` the reference's state_dict keys run through; rows are rows here, so it only holds the module"""

    def __init__(self, module):
        super().__init__()
        self._module = module


class Encoder(nn.Module):
    def __init__(self, in_dim, hidden, lod, enc_var_activation):
        super().__init__()
        self._hidden_layers = _blocks([in_dim, hidden, hidden, hidden])
        self._mean_layer = nn.Linear(hidden, lod)
        self._log_var_layer = nn.Linear(hidden, lod)
        self.enc_var_activation = enc_var_activation

    def forward(self, obs):
        h = _stack(self._hidden_layers, obs)
        h = F.normalize(h, p=2, dim=-1, eps=1e-8)      # output normalisation "pre": after the last hidden layer
        mean = linear(h, self._mean_layer.weight, self._mean_layer.bias)
        return mean, _variance(linear(h, self._log_var_layer.weight, self._log_var_layer.bias), self.enc_var_activation)


class SplitDiagGaussianDecoder(nn.Module):
    def __init__(self, lod, hidden, out_dim, dec_var_activation):
        super().__init__()
        self.dec_var_activation = dec_var_activation
        self._hidden_layers_mean = _blocks([2 * lod, hidden, hidden, hidden])
        self._hidden_layers_var = _blocks([3 * lod, hidden])
        self._out_layer_mean = nn.Linear(hidden, out_dim)
        self._out_layer_var = nn.Linear(hidden, out_dim)

    def mean(self, latent_mean):
        return linear(_stack(self._hidden_layers_mean, latent_mean), self._out_layer_mean.weight, self._out_layer_mean.bias)


class Physionet_USHCN(nn.Module):
    def __init__(self, target_dim, lsd, args, use_cuda_if_available=True):
        super().__init__()
        self.hidden_units = args.hidden_units
        self.target_dim = target_dim
        self._lsd = lsd
        if lsd % 2 != 0:
            raise Exception("Latent state dimension must be even number.")
        self._lod = lsd // 2
        self.args = args
        self._initial_state_variance = 10.0
        self._cru_layer = CRULayer(latent_obs_dim=self._lod, args=args)
        enc = Encoder(target_dim, self.hidden_units, self._lod, args.enc_var_activation)      # drawn before the decoder, registered after
        self._dec = TimeDistributed(SplitDiagGaussianDecoder(self._lod, self.hidden_units, target_dim, args.dec_var_activation))
        self._enc = TimeDistributed(enc)
        init = float(np.log(np.exp(self._initial_state_variance) - 1.0))
        self._log_icu = nn.Parameter(init * torch.ones(1, self._lod))
        self._log_icl = nn.Parameter(init * torch.ones(1, self._lod))

    def initial_covariance(self):
        return torch.log(torch.exp(self._log_icu) + 1.0), torch.log(torch.exp(self._log_icl) + 1.0)


class CRU(nn.Module):
    def __init__(self, configs):
        super().__init__()
        self.input_len = configs.input_len
        self.pred_len = configs.pred_len
        self.enc_in = configs.enc_in
        self.device = configs.device if isinstance(configs.device, torch.device) else torch.device(configs.device)

        class CRU_Args_Internal:
            def __init__(self):
                self.latent_state_dim = getattr(configs, "cru_lsd", 32)
                self.hidden_units = getattr(configs, "cru_hidden_units", 32)
                self.enc_num_layers = getattr(configs, "cru_enc_num_layers", 1)
                self.dec_num_layers = getattr(configs, "cru_dec_num_layers", 1)
                self.num_cru_layers = getattr(configs, "cru_num_layers", 1)
                self.dropout_type = getattr(configs, "cru_dropout_type", "None")
                self.dropout_rate = getattr(configs, "cru_dropout_rate", 0.0)
                self.use_gate_hidden_states = getattr(configs, "cru_use_gate_hidden_states", True)
                self.use_ode_for_gru = getattr(configs, "cru_use_ode_for_gru", False)
                self.use_decay_gravity_gate = getattr(configs, "cru_use_decay_gravity_gate", True)
                self.use_gravity_gate = getattr(configs, "cru_use_gravity_gate", True)
                self.use_decay_input_gate = getattr(configs, "cru_use_decay_input_gate", True)
                self.use_input_gate = getattr(configs, "cru_use_input_gate", True)
                self.use_skip_connection = getattr(configs, "cru_use_skip_connection", True)
                self.solver = getattr(configs, "cru_solver", "euler")
                self.extrapolation = True
                self.device = configs.device
                self.batch_size = configs.batch_size
                self.lr = getattr(configs, "lr", 1e-3)
                self.rkn = getattr(configs, "cru_rkn", False)
                self.f_cru = getattr(configs, "cru_f_cru", False)
                self.bandwidth = getattr(configs, "cru_bandwidth", 3)
                self.num_basis = getattr(configs, "cru_num_basis", 15)
                self.trans_net_hidden_units = getattr(configs, "cru_trans_net_hidden_units", [])
                self.trans_net_hidden_activation = getattr(configs, "cru_trans_net_hidden_activation", "elup1")
                self.t_sensitive_trans_net = getattr(configs, "cru_t_sensitive_trans_net", False)
                self.trans_var_activation = getattr(configs, "cru_trans_var_activation", "elup1")
                self.trans_covar = getattr(configs, "cru_trans_covar", 0.1)
                self.enc_var_activation = getattr(configs, "cru_enc_var_activation", "square")
                self.dec_var_activation = getattr(configs, "cru_dec_var_activation", "exp")

        args = CRU_Args_Internal()
        self.cru_model_core = Physionet_USHCN(target_dim=self.enc_in, lsd=args.latent_state_dim, args=args,
                                              use_cuda_if_available=(self.device.type == "cuda")).to(self.device)
        self.fused_calls = 0         # forecasting() calls whose recurrence took the fused HIP path (tests assert which path ran)

    @property
    def immtsf_graphable(self):
        """forecasting() can be captured into a graph where the recurrence is the fused kernel or the discrete cell: the composed
        continuous cell calls torch.matrix_exp, which reads a batch's norms on the host"""
        a = self.cru_model_core.args
        return bool(a.rkn or (config.cru_fused and not a.t_sensitive_trans_net and len(a.trans_net_hidden_units) == 0 and
                              cru_supported(self.cru_model_core._lsd, a.num_basis, a.bandwidth, 1)))

    def _scan_params(self):
        core = self.cru_model_core
        cell = core._cru_layer._cell
        return cell.bases() + (cell._coefficient_net[0].weight, cell._coefficient_net[0].bias, cell._log_transition_noise, core._log_icu,
                               core._log_icl)

    def _fused_ok(self, tp_to_predict, data, tp, mask):
        core = self.cru_model_core
        a = core.args
        B, L, _ = data.shape
        if not (config.cru_fused and not a.rkn and not a.f_cru and not a.t_sensitive_trans_net and len(a.trans_net_hidden_units) == 0 and
                B > 0 and L > 0 and all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in (tp_to_predict, data, tp, mask))
                and cru_supported(core._lsd, a.num_basis, a.bandwidth, L + tp_to_predict.shape[1])
                and B * (L + tp_to_predict.shape[1]) * core._lsd < 1 << 31):
            return False
        # the module itself: a .half() / .bfloat16() model, one left on another device -> composed
        return all(q.device == data.device and q.dtype == torch.float32 for q in self._scan_params())

    @_fp32_entry
    def forecasting(self, tp_to_predict, observed_data, observed_tp, observed_mask):
        core = self.cru_model_core
        cell = core._cru_layer._cell
        B, L, C = observed_data.shape
        Lp = tp_to_predict.shape[1]
        lod = core._lod
        t = torch.cat((observed_tp, tp_to_predict), dim=1).float()
        valid = torch.cat((observed_mask.any(dim=-1), torch.zeros(B, Lp, device=observed_mask.device, dtype=torch.bool)), dim=1)
        y, y_var = core._enc._module(observed_data.float().reshape(B * L, C))
        pad = torch.zeros(B, Lp, lod, device=y.device, dtype=y.dtype)      # the horizon's observations are never read: no encoder rows for them
        y, y_var = torch.cat((y.view(B, L, lod), pad), 1), torch.cat((y_var.view(B, L, lod), pad), 1)
        icu, icl = core.initial_covariance()
        if self._fused_ok(tp_to_predict, observed_data, observed_tp, observed_mask):
            self.fused_calls += 1
            post_mean = cru_scan(y, y_var, valid, t, core.args.bandwidth, *cell.bases(), cell._coefficient_net[0].weight,
                                 cell._coefficient_net[0].bias, cell.transition_variance(), icu, icl)[0]
        else:
            zeros = torch.zeros(1, lod, device=y.device, dtype=torch.float32)
            post_mean = core._cru_layer(y, y_var, torch.zeros(1, core._lsd, device=y.device, dtype=torch.float32), [icu, icl, zeros], valid, t)
        out = core._dec._module.mean(post_mean[:, L:, :].reshape(B * Lp, core._lsd))
        return out.view(B, Lp, C)


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
