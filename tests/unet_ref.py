"""Float64 restatement of the recurrent U-Nets (ebfi_amd.unet: UNetFlow, UNetRecurrent, SRUNetRecurrent), written from the law
in include/ebfi_hip.h (section "models/model_misc/unet.py") and the module docstrings, not from the reference's file: plain
tensors under their state-dict names, torch.nn.functional's conv2d / interpolate / pad and autograd for the derivatives, the
cell equations spelled out.  `dtype=torch.float32` runs the same operations in float32: the yardstick the GPU tests measure the
native path against.

  CASES                          the five configurations of tests/golden/unet_small.npz
  unet_kwargs(case)              the dict the module classes are built from
  names_and_shapes(case)         the state-dict entries, in order
  fill_state(seed, case)         every parameter from numpy.random.RandomState(seed), rounded to float32 values
  make_inputs(seed, case)        two inputs and two cotangents, float32 values
  run(case, state, xs, cots)     two consecutive calls with the state carried, loss = sum(cot1 * out1) + sum(cot2 * out2), one
                                 backward -> {'outs', 'states', 'grads', 'preacts'}
"""
import numpy as np
import torch
import torch.nn.functional as F

CFG = dict(base_num_channels=8, num_encoders=2, num_residual_blocks=1, num_bins=5, norm=None, use_upsample_conv=True, kernel_size=3)
CASES = {
    "A": dict(net="UNetFlow", recurrent_block_type="convlstm", skip_type="sum", shape=(2, 5, 16, 24)),
    "B": dict(net="UNetFlow", recurrent_block_type="convgru", skip_type="sum", shape=(2, 5, 18, 22)),
    "C": dict(net="UNetFlow", recurrent_block_type="convlstm", skip_type="concat", shape=(1, 5, 18, 22)),
    "D": dict(net="UNetRecurrent", recurrent_block_type="convgru", skip_type="sum", shape=(2, 5, 10, 14), final_activation="sigmoid"),
    "E": dict(net="SRUNetRecurrent", recurrent_block_type="convlstm", skip_type="sum", shape=(1, 5, 10, 14), num_output_channels=2),
}


def unet_kwargs(case):
    c = CASES[case]
    kw = dict(CFG, skip_type=c["skip_type"], recurrent_block_type=c["recurrent_block_type"])
    for k in ("final_activation", "num_output_channels"):
        if k in c:
            kw[k] = c[k]
    return kw


def out_channels(case):
    return {"UNetFlow": 3, "UNetRecurrent": 1}.get(CASES[case]["net"], CASES[case].get("num_output_channels"))


def _widths():
    base, n = CFG["base_num_channels"], CFG["num_encoders"]
    return [base * 2 ** i for i in range(n)], [base * 2 ** (i + 1) for i in range(n)]


def names_and_shapes(case):
    c = CASES[case]
    k, base = CFG["kernel_size"], CFG["base_num_channels"]
    ins, outs = _widths()
    skipw = (lambda ch: ch) if c["skip_type"] == "sum" else (lambda ch: 2 * ch)
    conv = lambda name, co, ci, kk: [(name + ".weight", (co, ci, kk, kk)), (name + ".bias", (co,))]
    out = conv("head.conv2d", base, CFG["num_bins"], k)
    for i, (ci, co) in enumerate(zip(ins, outs)):
        out += conv("encoders.%d.conv.conv2d" % i, co, ci, k)
        if c["recurrent_block_type"] == "convlstm":
            out += conv("encoders.%d.recurrent_block.Gates" % i, 4 * co, 2 * co, 3)
        else:
            for g in ("reset_gate", "update_gate", "out_gate"):
                out += conv("encoders.%d.recurrent_block.%s" % (i, g), co, 2 * co, 3)
    for j in range(CFG["num_residual_blocks"]):
        out += conv("resblocks.%d.conv1" % j, outs[-1], outs[-1], 3) + conv("resblocks.%d.conv2" % j, outs[-1], outs[-1], 3)
    for i, (ci, co) in enumerate(zip(reversed(outs), reversed(ins))):
        out += conv("decoders.%d.conv2d" % i, co, skipw(ci), k)
    if c["net"] == "SRUNetRecurrent":
        for i, ch in enumerate(outs[::-1] + [base]):
            out += conv("skip_upsampler.%d.conv2d" % i, ch, skipw(ch), k)
    return out + conv("pred.conv2d", out_channels(case), skipw(base), 1)


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32).astype(np.float64))


def fill_state(seed, case):
    """{name: float64 tensor holding float32 values}: weights normal with standard deviation 1 / sqrt(fan-in), biases 0.1 normal."""
    rs = np.random.RandomState(seed)
    state = {}
    for name, shape in names_and_shapes(case):
        if name.endswith("bias"):
            state[name] = _f32(0.1 * rs.standard_normal(shape))
        else:
            state[name] = _f32(rs.standard_normal(shape) / np.sqrt(np.prod(shape[1:])))
    return state


def out_shape(case):
    B, _, H, W = CASES[case]["shape"]
    s = 2 if CASES[case]["net"] == "SRUNetRecurrent" else 1
    return (B, out_channels(case), s * H, s * W)


def make_inputs(seed, case, calls=2):
    rs = np.random.RandomState(seed)
    xs = [_f32(rs.standard_normal(CASES[case]["shape"])) for _ in range(calls)]
    cots = [_f32(rs.standard_normal(out_shape(case))) for _ in range(calls)]
    return xs, cots


def _fit(x1, x2):
    dy, dx = x2.shape[2] - x1.shape[2], x2.shape[3] - x1.shape[3]
    return F.pad(x1, (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))


def sigmoid(v):
    return 1 / (1 + torch.exp(-v))


class RefUNet:
    def __init__(self, case, weights):
        self.case, self.c, self.w = case, CASES[case], weights
        self.states = [None] * CFG["num_encoders"]
        self.preacts = []              # the pre-activation of every ReLU, detached

    def conv(self, x, name, stride=1, relu=True):
        w = self.w[name + ".weight"]
        y = F.conv2d(x, w, self.w[name + ".bias"], stride, w.shape[-1] // 2)
        return self.relu(y) if relu else y

    def relu(self, y):
        self.preacts.append(y.detach())
        return torch.where(y > 0, y, torch.zeros_like(y))

    def skip(self, x1, x2):
        x1 = _fit(x1, x2)
        return x1 + x2 if self.c["skip_type"] == "sum" else torch.cat([x1, x2], 1)

    def up_conv(self, x, name, scale):
        return self.conv(F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False), name)

    def cell(self, x, prefix, state):
        zeros = torch.zeros_like(x)
        if self.c["recurrent_block_type"] == "convlstm":
            h, cprev = state if state is not None else (zeros, zeros)
            gi, gf, go, gc = self.conv(torch.cat([x, h], 1), prefix + ".Gates", relu=False).chunk(4, 1)
            cell = sigmoid(gf) * cprev + sigmoid(gi) * torch.tanh(gc)
            hidden = sigmoid(go) * torch.tanh(cell)
            return hidden, (hidden, cell)
        h = state if state is not None else zeros
        stacked = torch.cat([x, h], 1)
        u = sigmoid(self.conv(stacked, prefix + ".update_gate", relu=False))
        r = sigmoid(self.conv(stacked, prefix + ".reset_gate", relu=False))
        o = torch.tanh(self.conv(torch.cat([x, h * r], 1), prefix + ".out_gate", relu=False))
        new = h * (1 - u) + o * u
        return new, new

    def call(self, x):
        n = CFG["num_encoders"]
        sr = self.c["net"] == "SRUNetRecurrent"
        x = head = self.conv(x, "head.conv2d")
        blocks = []
        for i in range(n):
            x = self.conv(x, "encoders.%d.conv.conv2d" % i, stride=2)
            x, self.states[i] = self.cell(x, "encoders.%d.recurrent_block" % i, self.states[i])
            blocks.append(x)
        for j in range(CFG["num_residual_blocks"]):
            y = self.conv(x, "resblocks.%d.conv1" % j)
            x = self.relu(self.conv(y, "resblocks.%d.conv2" % j, relu=False) + x)
        for i in range(n):
            skip = blocks[n - i - 1]
            if sr:
                skip = self.up_conv(skip, "skip_upsampler.%d.conv2d" % i, 2)
            x = self.up_conv(self.skip(x, skip), "decoders.%d.conv2d" % i, 4 if sr and i == 0 else 2)
        if sr:
            head = self.up_conv(head, "skip_upsampler.%d.conv2d" % n, 2)
        out = self.conv(self.skip(x, head), "pred.conv2d", relu=False)
        return sigmoid(out) if self.c.get("final_activation") == "sigmoid" else out


def flat_states(states):
    out = []
    for s in states:
        out += list(s) if isinstance(s, (tuple, list)) else [s]
    return out


def run(case, state, xs, cots, dtype=torch.float64):
    names = [n for n, _ in names_and_shapes(case)]
    w = {n: state[n].to(dtype).clone().requires_grad_(True) for n in names}
    net = RefUNet(case, w)
    outs = [net.call(x.to(dtype)) for x in xs]
    loss = sum((c.to(dtype) * o).sum() for c, o in zip(cots, outs))
    grads = torch.autograd.grad(loss, [w[n] for n in names])
    return {"outs": [o.detach() for o in outs], "states": [s.detach() for s in flat_states(net.states)],
            "grads": dict(zip(names, grads)), "preacts": net.preacts}


def module_outputs(out):
    """What a module call returns -> the tensor run() calls `out`: UNetFlow's dict is cat(image, flow)."""
    return torch.cat([out["image"], out["flow"]], 1) if isinstance(out, dict) else out


def grad_table(grads):
    """float64 [P, 9]: the sum, then the first 8 elements (zero-padded), of every gradient -- what the fixture keeps of them."""
    table = np.zeros((len(grads), 9))
    for i, g in enumerate(grads):
        g = g.detach().double().cpu().reshape(-1)
        table[i, 0] = float(g.sum())
        table[i, 1:1 + min(8, g.numel())] = g[:8].numpy()
    return table
