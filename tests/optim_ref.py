"""The optimiser step of the training closure restated in numpy -- the gradient clip of torch/lib/run_epoch.lua:304-312, weight
decay, torch/lib/adam.lua:53-68 and torch/lib/rmsprop.lua:43-54 -- in fp64 (the reference of tests/test_hip_optim.py) and in
fp32 with the operation order of tfl_optim_step (the witness: what the bound leaves room for), plus the broken variants the
bound has to catch. tests/test_optim_ref_cpu.py holds the fp32 form inside the bound and every variant outside it."""
import numpy as np

ADAM, RMSPROP = "adam", "rmsprop"
VARIANTS = ("eps-inside-root", "no-bias-correction", "clip-by-squared-norm", "decay-after-moments", "t-incremented-before-clr")
BAR = 1e-5

# (parameter set, method, clip active): epsilon = 1e-4 is the reference's default (default_conf.lua:115); weightDecay and
# learningRateDecay non-zero so that both terms act; initialMean small against the squared gradients' mean (a large one
# would swamp them in RMSprop's mean square, and nothing done to the gradients could show there)
CASES = [(kind, method, clip) for kind in ("yang", "default2d") for method in (ADAM, RMSPROP) for clip in (True, False)]
STEPS = 3


def config(method, clip):
    c = dict(method=method, learningRate=0.0025, learningRateDecay=0.05, beta1=0.9, beta2=0.999, epsilon=1e-4, weightDecay=0.01,
             alpha=0.99, initialMean=1e-6, gradNormThreshold=0.1 if clip else 0.0)
    return c


def parameters(kind):
    """[w0, b0, w1, b1, ...] of the seeded `yang` (2-D) / 2-D `default` model, float32"""
    import model_grad_ref as R
    m = R.make_model("yang" if kind == "yang" else "default", False, seed=3)
    return [np.array(t, np.float32) for wb in m.layers for t in wb]


def gradients(kind, step):
    """random gradients of the parameters' shapes: norm well above the clip threshold of config() (0.05 per element over
    >= 259 elements: >= 0.8 against 0.1), so that rounding cannot flip the clip decision"""
    rng = np.random.RandomState(1000 + step + (0 if kind == "yang" else 50))
    return [(rng.randn(*p.shape) * 0.05).astype(np.float32) for p in parameters(kind)]


def applies(variant, cfg):
    if variant in ("no-bias-correction", "t-incremented-before-clr"):
        return cfg["method"] == ADAM
    if variant == "clip-by-squared-norm":
        return cfg["gradNormThreshold"] > 0
    return True


def new_state(params, cfg, dtype=np.float64):
    fill = cfg["initialMean"] if cfg["method"] == RMSPROP else 0.0
    return dict(t=0, m=[np.full(p.shape, fill, dtype) for p in params], v=[np.zeros(p.shape, dtype) for p in params])


def step(x, g, state, cfg, dtype=np.float64, variant=None):
    """one step on the tensor lists x, g (not modified): (new x, the clipped and decayed g). state (t, m, v) is advanced in
    place. dtype float64: everything in fp64. float32: each element operation rounded to fp32 in the order of the reference's
    tensor calls; the scalars as tfl_optim_step forms them (the norm summed in fp64, norm / threshold and stepSize formed in
    fp64 and rounded once)."""
    f = dtype
    x = [np.asarray(a, f) for a in x]
    g = [np.asarray(a, f) for a in g]
    thr = cfg["gradNormThreshold"]
    if thr > 0:
        ss = sum(float((a.astype(np.float64) ** 2).sum()) for a in g)
        norm = ss if variant == "clip-by-squared-norm" else np.sqrt(ss)
        if norm > thr:
            g = [a / f(norm / thr) for a in g]
    wd = f(cfg["weightDecay"])
    late_decay = variant == "decay-after-moments"
    gm = g                                      # what the moments see
    if wd != 0:
        g = [a + wd * b for a, b in zip(g, x)]
        if not late_decay:
            gm = g
    eps = f(cfg["epsilon"])
    t0 = state["t"]
    state["t"] = t0 + 1
    if cfg["method"] == ADAM:
        b1, b2 = cfg["beta1"], cfg["beta2"]
        tc = t0 + 1 if variant == "t-incremented-before-clr" else t0
        clr = cfg["learningRate"] / (1.0 + tc * cfg["learningRateDecay"])
        t1 = t0 + 1
        step_size = clr if variant == "no-bias-correction" else clr * np.sqrt(1.0 - b2 ** t1) / (1.0 - b1 ** t1)
        ns = f(-step_size)
        out = []
        for i, (xi, gi) in enumerate(zip(x, gm)):
            m = state["m"][i] * f(b1) + f(1.0 - b1) * gi
            v = state["v"][i] * f(b2) + (f(1.0 - b2) * gi) * gi
            state["m"][i], state["v"][i] = m, v
            denom = np.sqrt(v + eps) if variant == "eps-inside-root" else np.sqrt(v) + eps
            out.append(xi + (ns * m) / denom)
        return out, g
    a = cfg["alpha"]
    ns = f(-cfg["learningRate"])
    out = []
    for i, (xi, gi, gmi) in enumerate(zip(x, g, gm)):
        m = state["m"][i] * f(a)
        m = m + (f(1.0 - a) * gmi) * gmi
        state["m"][i] = m
        denom = np.sqrt(m + eps) if variant == "eps-inside-root" else np.sqrt(m) + eps
        out.append(xi + (ns * gi) / denom)
    return out, g


def l2(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))


def within(x, x64, prev64):
    """the bound on an updated parameter tensor: |x - x64| <= 1e-5 |delta64| + 2^-24 |x64| (L2), delta64 = the step's fp64
    update. The first term is the project's 1e-5 bar applied to the UPDATE (held to the parameter it would hide any error: a
    step moves a parameter by ~1e-3 of itself); the second is the rounding of the stored fp32 value. Returns (error, bound)."""
    x64 = np.asarray(x64, np.float64)
    err = l2(np.asarray(x, np.float64) - x64)
    return err, BAR * l2(x64 - np.asarray(prev64, np.float64)) + 2.0 ** -24 * l2(x64)


def rel(a, b):
    """plain rel-L2 of a against the fp64 b (m, v, the clipped gradients)"""
    d = l2(b)
    return l2(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / d if d > 0 else l2(a)


def trajectory(kind, cfg, dtype=np.float64, variant=None, steps=STEPS):
    """[(x, g', m, v)] after each of `steps` steps from the seeded parameters with gradients(kind, step)"""
    x = [np.asarray(p, dtype) for p in parameters(kind)]
    st = new_state(x, cfg, dtype)
    out = []
    for s in range(steps):
        x, g = step(x, gradients(kind, s), st, cfg, dtype, variant)
        out.append((x, g, [a.copy() for a in st["m"]], [a.copy() for a in st["v"]]))
    return out


def check(got, want, start, adam):
    """got / want: trajectories; the worst (error / bound) over the parameter tensors and the worst rel-L2 of m, v, g' --
    both <= 1 and <= BAR for a pass. Returns (worst_x_ratio, worst_state_rel)."""
    worst_x, worst_s = 0.0, 0.0
    prev = start
    for (x, g, m, v), (x64, g64, m64, v64) in zip(got, want):
        for a, b, p in zip(x, x64, prev):
            err, bound = within(a, b, p)
            worst_x = max(worst_x, err / bound)
        for a, b in list(zip(g, g64)) + list(zip(m, m64)) + (list(zip(v, v64)) if adam else []):
            worst_s = max(worst_s, rel(a, b))
        prev = x64
    return worst_x, worst_s
