"""The checker for SGU2 training: a plain torch CPU restatement of the
reference's loop (models/GateUnits.py:66-114) -- SGU2Model's nn.LSTM + Linear,
an explicit ``h * keep * 5`` in place of Dropout(0.8), nn.MSELoss,
torch.optim.Adam with default settings, the validation pass and the early
stopping rule -- in float32 or float64, driven by an explicit schedule
(perm[epochs, n]: the sample at each position of the epoch; keep[epochs, n, H]:
its dropout mask).  Nothing here shares code with csrc/."""
import numpy as np
import torch

KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc.weight", "fc.bias")
M = 8                                  # the margin of every comparison (see tolerance())
EPS32 = float(np.finfo(np.float32).eps)
MIN_GRAD = 1e-6                        # |g| of the float64 reference: exactly 0 or at least this


def n_params(hidden):
    return 4 * hidden + 4 * hidden * hidden + 8 * hidden + hidden + 1


def rand_weights(hidden, gain=1.0, seed=0):
    """Flat weights of scale gain / sqrt(H), as tests/test_sgu2.py draws them."""
    rng = np.random.default_rng([seed, hidden, int(gain)])
    return (rng.uniform(-1, 1, n_params(hidden)) / np.sqrt(hidden) * gain).astype(np.float32)


class Net(torch.nn.Module):
    def __init__(self, hidden, dtype):
        super().__init__()
        self.lstm = torch.nn.LSTM(1, hidden, batch_first=True, dtype=dtype)
        self.fc = torch.nn.Linear(hidden, 1, dtype=dtype)

    def forward(self, x, keep5=None):
        out, _ = self.lstm(x)
        h = out[:, -1, :]
        if keep5 is not None:
            h = h * keep5
        return self.fc(h)


def make_net(w, hidden, dtype):
    net = Net(hidden, dtype)
    sd = net.state_dict()
    o = 0
    for k in KEYS:
        m = sd[k].numel()
        sd[k].copy_(torch.as_tensor(np.asarray(w[o:o + m]), dtype=dtype).reshape(sd[k].shape))
        o += m
    return net


def flat(net, grad=False):
    ps = dict(net.named_parameters())
    return np.concatenate([(ps[k].grad if grad else ps[k]).detach().reshape(-1).numpy().astype(np.float64)
                           for k in KEYS])


def _x(X, dtype):
    X = torch.as_tensor(np.asarray(X, np.float32)).to(dtype)
    return X.reshape(X.shape[0], -1, 1)


def loss_grad(w, hidden, X, y, keep=None, dtype=torch.float64, label_scale=1.0):
    """(loss, flat gradient) of one minibatch by autograd; keep [n, H] 0/1 or None (eval mode)."""
    net = make_net(w, hidden, dtype)
    yt = torch.as_tensor(np.asarray(y, np.float32)).to(dtype).reshape(-1, 1) * label_scale
    k5 = None if keep is None else torch.as_tensor(np.asarray(keep, np.float32)).to(dtype) * 5.0
    loss = torch.nn.functional.mse_loss(net(_x(X, dtype), k5), yt)
    loss.backward()
    return float(loss.detach()), flat(net, grad=True)


def train(w, hidden, Xt, yt, Xv, yv, perm, keep, batch, epochs, lr, dtype=torch.float64, patience=5,
          label_scale=1.0):
    """The reference's loop under an explicit schedule.  Returns dict(train_loss,
    val_loss (lists of Python floats), weights (flat float64), epochs_run,
    best_epoch, stopped, min_grad: the smallest non-zero |g| any Adam step saw)."""
    net = make_net(w, hidden, dtype)
    Xt, Xv = _x(Xt, dtype), _x(Xv, dtype)
    yt = torch.as_tensor(np.asarray(yt, np.float32)).to(dtype).reshape(-1, 1) * label_scale
    yv = torch.as_tensor(np.asarray(yv, np.float32)).to(dtype).reshape(-1, 1) * label_scale
    n = Xt.shape[0]
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    crit = torch.nn.MSELoss()
    best, trig, best_epoch, stopped = float("inf"), 0, -1, False
    hist = {"train_loss": [], "val_loss": []}
    min_grad = np.inf
    for e in range(epochs):
        total, nb = 0.0, 0
        for p0 in range(0, n, batch):
            idx = torch.as_tensor(np.asarray(perm[e][p0:p0 + batch], np.int64))
            k5 = torch.as_tensor(np.asarray(keep[e][p0:p0 + batch], np.float32)).to(dtype) * 5.0
            opt.zero_grad()
            loss = crit(net(Xt[idx], k5), yt[idx])
            loss.backward()
            g = np.abs(flat(net, grad=True))
            if np.any(g > 0):
                min_grad = min(min_grad, float(g[g > 0].min()))
            opt.step()
            total += loss.item()
            nb += 1
        with torch.no_grad():
            val = crit(net(Xv), yv).item() if Xv.shape[0] else float("nan")
        hist["train_loss"].append(total / nb)
        hist["val_loss"].append(val)
        if val < best:
            best, best_epoch, trig = val, e, 0
        else:
            trig += 1
            if trig >= patience:
                stopped = True
                break
    return dict(hist, weights=flat(net), epochs_run=len(hist["val_loss"]), best_epoch=best_epoch, stopped=stopped,
                min_grad=min_grad)


def tolerance(ref32, ref64):
    """M * max(e_ref, float32 eps * scale) for one tensor: e_ref = max |float32
    reference - float64 reference|, scale = max |float64 reference|.  The margin
    M = 8 covers hardware exp2 / rcp (about one ulp worse than libm) and a batch
    reduction order that differs over up to 256 terms."""
    ref32, ref64 = np.asarray(ref32, np.float64).reshape(-1), np.asarray(ref64, np.float64).reshape(-1)
    e_ref = float(np.max(np.abs(ref32 - ref64))) if ref64.size else 0.0
    scale = float(np.max(np.abs(ref64))) if ref64.size else 0.0
    return M * max(e_ref, EPS32 * scale)


def ratio(got, ref32, ref64):
    """max |got - float64| / (tolerance / M): at most M passes, above M / 2 wants a look."""
    got, ref64 = np.asarray(got, np.float64).reshape(-1), np.asarray(ref64, np.float64).reshape(-1)
    err = float(np.max(np.abs(got - ref64))) if ref64.size else 0.0
    unit = tolerance(ref32, ref64) / M
    if unit == 0.0:  # an exactly zero tensor (W_hh's gradient at T = 1, a fully dropped h_T)
        return 0.0 if err == 0.0 else float("inf")
    return err / unit
