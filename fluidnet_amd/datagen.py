"""Training sets generated on the device: random scenes stepped with the PCG projection, every saved step a frame pair of
lib/data_binary.lua's layout -- into a resident frame store, onto the disk, or both.

    gconf = default_gconf(is3D=False, dims=(1, 128, 128))
    res = generate(gconf, "tr", nruns=320, seed=1, out_dir="data/datasets/my_set")      # then examples/train.py reads it
    res = generate(gconf, "tr", 8, 1, store=FrameStore(...)); tr = res["data"]            # or train on it without touching the disk

The reference's sets come from a Mantaflow fork and a scene script that are not part of its tree. THE SCENE PLAN HERE IS THIS
PROJECT'S OWN: it does not reproduce Manta's random stream, its wavelet noise or its scenes; what it shares with the reference
is the definition of a frame pair and the file layout.

A run is a sequence of states of simulate() with simMethod = 'pcg' (lib/simulate.lua:175-327): S_{k+1} = simulate(S_k). For every
saved step k (every saveEvery-th) one frame pair:
    NNNNNN_divergent.bin   (p, U, flags, density) of S_k after simulate(..., outputDiv=True): the state at simulate.lua:241-245,
                           p untouched, i.e. the previous solve's pressure
    NNNNNN.bin             (p, U, flags, density) of S_{k+1}: the same step carried through simulate.lua:247-326
produced as an outputDiv step, put_device of the divergent half, simulate.project, put_device of the target half -- the bits of
one full simulate() per step (tfl_simulate_project's contract).

plan_run is host code without a GPU; its draw order is part of the format of a (seed, run) pair (see plan_run). Runs are
stepped one at a time by default; generate(..., batch_runs=R) steps R of them as the items of one batch (simulate_items: per-item
forces, and with pcgPrecond 'mg' | 'none' one batched PCG solve in which every item keeps the iterations and the bits it has
alone) and holds the values of the set generated one run at a time.
"""
import ctypes
import os
import warnings

import numpy as np
import torch

from . import data as _data
from . import io as _io
from . import tfluids
from ._lib import TfluidsError, tfl_scene_prim
from .simulate import project, project_items, simulate, simulate_items

MAX_PRIMS = 32            # tfl_datagen.hpp kSceneMaxPrims
SPHERE, BOX = 0, 1
# The 3-D advection fast paths take |u dt| <= 0.9 cells for granted (a faster flow falls back to the gather kernels and lists
# every brick); the initial field and the emitters stay at half of that, which leaves the forces room to accelerate the flow.
REACH = 0.9
MAX_ATTEMPTS = 4          # sub-seeds tried for a run whose target divergence exceeds divThreshold


def default_gconf(is3D=False, dims=None, **over):
    """The generator's configuration. dt and advectionMethod are lib/default_conf.lua's (0.1, 'maccormack'); that file names no
    maccormackStrength, so the value of the reference's simulation script stands in (fluid_net_3d_sim.lua:79: 0.6). steps and
    saveEvery are the paper's recipe (256 steps, every 4th saved)."""
    g = dict(is3D=bool(is3D), dims=tuple(dims) if dims is not None else ((64, 64, 64) if is3D else (1, 128, 128)),
             steps=256, saveEvery=4, dt=0.1, advectionMethod="maccormack", maccormackStrength=0.6, maxIter=100,
             pcgPrecond="ic0",          # the preconditioner of every PCG solve of a run: 'none' | 'ilu0' | 'ic0' | 'mg' (tfluids.solveLinearSystemPCG)
             maxSpheres=3, maxBoxes=3, maxBlobs=3, maxEmitters=2, maxModels=1, models=(),
             # emitterSpeed: 0 (default): an emitter is a densityBC pair only. > 0: it also carries a UBC pair of that share of the
             # speed cap. A velocity imposed AFTER the projection leaves divergence on the emitter's surface, so such runs exceed
             # data.DIV_THRESHOLD: set divThreshold to None with it.
             emitterSpeed=0.0,
             noiseRadius=(2, 5), noisePasses=(1, 2), buoyancyProb=0.5, buoyancyScale=(0.5, 2.0),
             vorticityProb=0.5, vorticityConfinementAmp=(0.0, 0.8), divThreshold=_data.DIV_THRESHOLD)
    g.update(over)
    g["dims"] = tuple(int(v) for v in g["dims"])
    if not g["is3D"] and g["dims"][0] != 1:
        raise TfluidsError("2D domains should have unary z-dimension")
    return g


def _inside_np(prim, is3D, dims):
    """tfl_datagen.hpp scene_inside over a whole grid, in numpy float32 in the same order -> bool [Z, Y, X]"""
    Z, Y, X = dims
    cz = (np.arange(Z, dtype=np.float32) + np.float32(0.5)).reshape(Z, 1, 1)
    cy = (np.arange(Y, dtype=np.float32) + np.float32(0.5)).reshape(1, Y, 1)
    cx = (np.arange(X, dtype=np.float32) + np.float32(0.5)).reshape(1, 1, X)
    a, b = np.asarray(prim["a"], np.float32), np.asarray(prim["b"], np.float32)
    if prim["kind"] == SPHERE:
        dx, dy = cx - a[0], cy - a[1]
        d2 = dx * dx + dy * dy
        if is3D:
            dz = cz - a[2]
            d2 = d2 + dz * dz
        return np.broadcast_to(d2 <= b[0] * b[0], (Z, Y, X))
    ins = (cx >= a[0]) & (cx <= b[0]) & (cy >= a[1]) & (cy <= b[1])
    if is3D:
        ins = ins & (cz >= a[2]) & (cz <= b[2])
    return np.broadcast_to(ins, (Z, Y, X))


def _f32(v):
    return float(np.float32(v))


def _model_variants(model, index, dims):
    """the four orientations a plan may stamp a voxel model in -- io.flipDiagonal about axis 0, 1, 2 (where the array's other two
    dims are equal; else the array as it is) and unflipped -- each cropped to its bounding box; None where that box does not fit
    inside the grid's one-cell border. A model that fits in no orientation is refused by name; one without a set voxel too."""
    v = np.asarray(model, np.float32)
    if v.ndim != 3 or not (v != 0).any():
        raise TfluidsError("plan_run: voxel model %d is not a 3-D array with a set voxel" % index)
    out = []
    for flip in range(4):
        w = v
        if flip < 3 and len({v.shape[a] for a in range(3) if a != flip}) == 1:
            w = _io.flipDiagonal(v, flip)
        bb = _io.calculateBoundingBox(w)
        w = np.ascontiguousarray(w[bb["min"][0] - 1:bb["max"][0], bb["min"][1] - 1:bb["max"][1], bb["min"][2] - 1:bb["max"][2]])
        out.append(w if all(w.shape[a] <= dims[a] - 2 for a in range(3)) else None)
    if all(w is None for w in out):
        bb = _io.calculateBoundingBox(v)
        raise TfluidsError("plan_run: voxel model %d can never fit: its bounding box of %s voxels (z, y, x) exceeds the grid %s less its "
                           "one-cell border in every orientation" % (index, tuple(bb["max"][a] - bb["min"][a] + 1 for a in range(3)), tuple(dims)))
    return out


def plan_run(gconf, seed, run, attempt=0):
    """The scene of run `run`: a function of (gconf, seed, run, attempt) alone. numpy.random.RandomState([seed, run, attempt]),
    drawn in THIS order (every value rounded to float32 where it is stored):
      1. emitters: their number in [0, maxEmitters]; per emitter the radius, the centre (x, y[, z]), the density, and -- always
         drawn, used where emitterSpeed > 0 -- a direction (d normal draws) ;
      2. sphere obstacles: their number in [0, maxSpheres]; per sphere up to 16 tries of (radius, centre), the first that stays
         2 cells off the border and off every emitter is kept (none: the sphere is dropped);
      3. box obstacles: likewise, (half sizes, centre);
      4. voxel models (3-D, gconf['models'] = binvox arrays as io.loadVoxelData(...)['data']): their number in [0, maxModels];
         per model up to 16 tries of (index, flip axis or none, three offsets in +-0.2 of the grid, cut to those that keep the
         model's bounding box inside the one-cell border), stamped through io.flipDiagonal / padVoxelsToDims; a model whose
         bounding box fits in no orientation is refused by name;
      5. density blobs: their number in [1, maxBlobs]; per blob kind, size, centre, value;
      6. the noise: blur radius, passes, speed (the peak |component| of U_0 in cells per unit time, at most REACH / (2 dt));
      7. the gravity direction (one of the 2 d axis directions), buoyancyScale (0 with probability 1 - buoyancyProb) and
         vorticityConfinementAmp (0 with probability 1 - vorticityProb).
    -> a dict of plain numbers, lists and (voxels) one uint8 array."""
    is3D, (Z, Y, X) = bool(gconf["is3D"]), gconf["dims"]
    d = 3 if is3D else 2
    size = np.asarray([X, Y, Z][:d], np.float64)
    smin = float(size.min())
    rs = np.random.RandomState([int(seed) & 0xffffffff, int(run) & 0xffffffff, int(attempt)])
    cap = REACH / (2.0 * float(gconf["dt"]))

    def centre(margin):
        lo, hi = np.full(d, margin), size - margin
        c = lo + rs.uniform(size=d) * np.maximum(hi - lo, 0.0)
        return [_f32(v) for v in c] + ([0.0] if not is3D else [])

    # 1. emitters
    emitters = []
    for _ in range(int(rs.randint(0, int(gconf["maxEmitters"]) + 1))):
        r = _f32(rs.uniform(1.5, max(2.0, 0.05 * smin)))
        c = centre(r + 3.0)
        rho = _f32(rs.uniform(0.5, 1.0))
        dirn = rs.normal(size=d)
        dirn = dirn / max(float(np.linalg.norm(dirn)), 1e-6)
        vel = [_f32(v * cap * float(gconf["emitterSpeed"])) for v in dirn] + ([0.0] if not is3D else [])
        emitters.append(dict(kind=SPHERE, a=c, b=[r, 0.0, 0.0], val=rho, vel=vel))

    def clear_of_emitters(prim):
        # the primitive, grown by 2 cells, holds no cell of an emitter
        if prim["kind"] == SPHERE:
            grown = dict(prim, b=[prim["b"][0] + 2.0, 0.0, 0.0])
        else:
            grown = dict(prim, a=[v - 2.0 for v in prim["a"]], b=[v + 2.0 for v in prim["b"]])
        g = _inside_np(grown, is3D, (Z, Y, X))
        return not any((g & _inside_np(e, is3D, (Z, Y, X))).any() for e in emitters)

    obstacles = []
    # 2. spheres
    for _ in range(int(rs.randint(0, int(gconf["maxSpheres"]) + 1))):
        for _try in range(16):
            r = _f32(rs.uniform(max(1.5, 0.04 * smin), max(2.0, 0.12 * smin)))
            prim = dict(kind=SPHERE, a=centre(r + 3.0), b=[r, 0.0, 0.0], val=0.0)
            if 2.0 * (r + 3.0) < smin and clear_of_emitters(prim):
                obstacles.append(prim)
                break
    # 3. boxes
    for _ in range(int(rs.randint(0, int(gconf["maxBoxes"]) + 1))):
        for _try in range(16):
            half = [_f32(rs.uniform(max(1.0, 0.03 * s), max(1.5, 0.10 * s))) for s in size]
            c = centre(max(half) + 3.0)
            lo = [_f32(c[i] - half[i]) for i in range(d)] + ([0.0] if not is3D else [])
            hi = [_f32(c[i] + half[i]) for i in range(d)] + ([0.0] if not is3D else [])
            prim = dict(kind=BOX, a=lo, b=hi, val=0.0)
            if 2.0 * (max(half) + 3.0) < smin and clear_of_emitters(prim):
                obstacles.append(prim)
                break
    # 4. voxel models
    voxels = None
    models = list(gconf.get("models") or ())
    if is3D and models:
        variants = [_model_variants(m, i, (Z, Y, X)) for i, m in enumerate(models)]
        for _ in range(int(rs.randint(0, int(gconf["maxModels"]) + 1))):
            for _try in range(16):
                idx, flip = int(rs.randint(0, len(models))), int(rs.randint(0, 4))
                u = rs.uniform(-0.2, 0.2, size=3)
                v = variants[idx][flip]
                if v is None:      # this orientation's bounding box does not fit inside the one-cell border
                    continue
                # integer offsets from the centred position, at most 0.2 of the grid, cut to those that keep the pasted
                # bounding box inside the one-cell border: padVoxelsToDims pastes at floor((dim - box) / 2) + offset
                off = []
                for ax, dim in ((2, X), (1, Y), (0, Z)):
                    box = v.shape[ax]
                    centred = (dim - box) // 2
                    off.append(float(min(max(int(np.floor(u[2 - ax] * dim)), 1 - centred), dim - 1 - box - centred)))
                occ = _io.padVoxelsToDims(X, Y, Z, v, off[0], off[1], off[2]) != 0
                assert not (occ[[0, -1]].any() or occ[:, [0, -1]].any() or occ[:, :, [0, -1]].any())
                grown = occ.copy()      # 2 cells of clearance from every emitter, as for the primitives
                for _g in range(2):
                    g2 = grown.copy()
                    for ax in range(3):
                        g2 |= np.roll(grown, 1, ax) | np.roll(grown, -1, ax)
                    grown = g2
                if not any((grown & _inside_np(e, True, (Z, Y, X))).any() for e in emitters):
                    voxels = occ if voxels is None else (voxels | occ)
                    break
    # 5. blobs
    blobs = []
    for _ in range(int(rs.randint(1, int(gconf["maxBlobs"]) + 1))):
        kind = int(rs.randint(0, 2))
        r = _f32(rs.uniform(max(2.0, 0.06 * smin), max(3.0, 0.2 * smin)))
        c = centre(min(r + 2.0, smin / 2.0))
        val = _f32(rs.uniform(0.3, 1.0))
        if kind == SPHERE:
            blobs.append(dict(kind=SPHERE, a=c, b=[r, 0.0, 0.0], val=val))
        else:
            blobs.append(dict(kind=BOX, a=[_f32(v - r) for v in c[:d]] + ([0.0] if not is3D else []),
                              b=[_f32(v + r) for v in c[:d]] + ([0.0] if not is3D else []), val=val))
    # 6. the noise
    radius = int(rs.randint(int(gconf["noiseRadius"][0]), int(gconf["noiseRadius"][1]) + 1))
    passes = int(rs.randint(int(gconf["noisePasses"][0]), int(gconf["noisePasses"][1]) + 1))
    speed = _f32(rs.uniform(0.2, 1.0) * cap)
    # 7. the forces
    axis = int(rs.randint(0, 2 * d))
    gravity = [0.0, 0.0, 0.0]
    gravity[axis // 2] = 1.0 if axis % 2 == 0 else -1.0
    u1, b1, u2, v2 = rs.uniform(), rs.uniform(*gconf["buoyancyScale"]), rs.uniform(), rs.uniform(*gconf["vorticityConfinementAmp"])
    buoyancy = _f32(b1) if u1 < float(gconf["buoyancyProb"]) else 0.0
    vort = _f32(v2) if u2 < float(gconf["vorticityProb"]) else 0.0
    assert len(obstacles) <= MAX_PRIMS and len(blobs) <= MAX_PRIMS
    return dict(is3D=is3D, dims=(Z, Y, X), seed=int(seed), run=int(run), attempt=int(attempt), obstacles=obstacles, blobs=blobs,
                emitters=emitters, voxels=None if voxels is None else voxels.astype(np.uint8), noise_radius=radius,
                noise_passes=passes, speed=speed, gravity=gravity, buoyancyScale=buoyancy, vorticityConfinementAmp=vort,
                dt=float(gconf["dt"]), advectionMethod=gconf["advectionMethod"], maccormackStrength=float(gconf["maccormackStrength"]),
                maxIter=int(gconf["maxIter"]), pcgPrecond=str(gconf.get("pcgPrecond") or "ic0"))


def mconf_of(plan):
    """the mconf every step of the plan's run is simulated with"""
    return dict(dt=plan["dt"], advectionMethod=plan["advectionMethod"], maccormackStrength=plan["maccormackStrength"],
                buoyancyScale=plan["buoyancyScale"], gravityScale=0, vorticityConfinementAmp=plan["vorticityConfinementAmp"],
                gravity=list(plan["gravity"]), simMethod="pcg", maxIter=plan["maxIter"], pcgPrecond=plan.get("pcgPrecond") or "ic0")


def noise_seed(plan):
    """the (seed, run) words of the plan's noise: the attempt folded into the seed, so that a regenerated run gets new noise"""
    return (plan["seed"] + 0x632be5ab * plan["attempt"]) & 0xffffffff, plan["run"] & 0xffffffff


def _table(prims):
    arr = (tfl_scene_prim * max(len(prims), 1))()
    for i, p in enumerate(prims):
        arr[i].kind = int(p["kind"])
        for k in range(3):
            arr[i].a[k], arr[i].b[k] = float(p["a"][k]), float(p["b"][k])
        arr[i].val = float(p["val"])
    return arr


# ---- the scene kernels ---------------------------------------------------------------------------------------------------------
def scene_flags(obstacles, blobs, is3D, flags, density=None):
    """tfl_scene_flags: flags = emptyDomain(bnd = 1) + the obstacle primitives, density = the blobs (dicts kind / a / b / val)"""
    if len(obstacles) > MAX_PRIMS or len(blobs) > MAX_PRIMS:
        raise TfluidsError("scene_flags: at most %d primitives fit one table" % MAX_PRIMS)
    lib, ctx = tfluids._context(flags)
    tfluids._call(lib, ctx, lib.tfl_scene_flags(ctx, _table(obstacles), len(obstacles), _table(blobs), len(blobs), int(bool(is3D)),
                                                tfluids._tt5(flags), None if density is None else tfluids._tt5(density)))
    from .simulate import drop_wall_plan
    drop_wall_plan(flags)      # written through the library: torch's version counter has not moved


def noise_potential(seed, run, psi):
    """tfl_noise_potential: counter-based white noise in [-1, 1) into psi [B, 1 | 3, Z, Y, X]"""
    lib, ctx = tfluids._context(psi)
    tfluids._call(lib, ctx, lib.tfl_noise_potential(ctx, int(seed) & 0xffffffff, int(run) & 0xffffffff, tfluids._tt5(psi)))


def curl_mac(psi, amp, is3D, U):
    """tfl_curl_mac: U = amp * the MAC-staggered curl of psi"""
    lib, ctx = tfluids._context(psi)
    tfluids._call(lib, ctx, lib.tfl_curl_mac(ctx, tfluids._tt5(psi), float(amp), int(bool(is3D)), tfluids._tt5(U)))


def initial_velocity(plan, device):
    """U_0 before the walls: noise -> `passes` box blurs of radius r -> curl at amp = 1 -> its peak |component| m (read back: once
    per run) -> curl at amp = float32(speed) / m. -> (U [1, C, Z, Y, X], amp)"""
    is3D, (Z, Y, X) = plan["is3D"], plan["dims"]
    psi = torch.empty(1, 3 if is3D else 1, Z, Y, X, device=device)
    tmp = torch.empty_like(psi)
    noise_potential(*noise_seed(plan), psi)
    for _ in range(plan["noise_passes"]):
        tfluids.rectangularBlur(psi, plan["noise_radius"], is3D, tmp)
        psi, tmp = tmp, psi
    U = torch.empty(1, 3 if is3D else 2, Z, Y, X, device=device)
    curl_mac(psi, 1.0, is3D, U)
    peak = np.float32(U.abs().max().item())
    amp = float(np.float32(plan["speed"]) / peak) if peak > 0 else 0.0
    curl_mac(psi, amp, is3D, U)
    return U, amp


def emitter_pairs(plan):
    """the emitters as host arrays: (UBC, UBCInvMask) or (None, None) where no emitter carries a velocity, and (densityBC,
    densityBCInvMask) or (None, None) without emitters -- [1, C | 1, Z, Y, X] float32"""
    is3D, dims = plan["is3D"], plan["dims"]
    if not plan["emitters"]:
        return (None, None), (None, None)
    C = 3 if is3D else 2
    dbc, dmk = np.zeros((1, 1) + dims, np.float32), np.ones((1, 1) + dims, np.float32)
    ubc, umk = np.zeros((1, C) + dims, np.float32), np.ones((1, C) + dims, np.float32)
    moving = False
    for e in plan["emitters"]:
        ins = _inside_np(e, is3D, dims)
        dbc[0, 0][ins], dmk[0, 0][ins] = np.float32(e["val"]), 0.0
        if any(v != 0.0 for v in e["vel"]):
            moving = True
            for c in range(C):
                ubc[0, c][ins], umk[0, c][ins] = np.float32(e["vel"][c]), 0.0
    return ((ubc, umk) if moving else (None, None)), (dbc, dmk)


def init_state(plan, device):
    """S_0 of the plan as a batch of simulate(): flags (k_scene_flags + the voxel models stamped on the host side), the density
    blobs, U_0 = the noise field -> setWallBcs -> one PCG projection (frame 0 starts divergence-free with respect to the walls),
    pDiv = 0, and the emitters as BC pairs."""
    is3D, dims = plan["is3D"], plan["dims"]
    device = torch.device(device)
    flags = torch.empty((1, 1) + dims, device=device)
    density = torch.empty_like(flags)
    scene_flags(plan["obstacles"], plan["blobs"], is3D, flags, density)
    if plan.get("voxels") is not None:
        occ = torch.from_numpy(plan["voxels"].astype(np.bool_)).to(device).view(flags.shape)
        flags.masked_fill_(occ, 2.0)
        density.masked_fill_(occ, 0.0)
    U, _ = initial_velocity(plan, device)
    p = torch.zeros_like(flags)
    div = torch.empty_like(flags)
    tfluids.setWallBcsForward(U, flags)
    tfluids.velocityDivergenceForward(U, flags, div)
    tfluids.solveLinearSystemPCG(p, flags, div, is3D, 1e-4, plan["maxIter"], plan.get("pcgPrecond") or "ic0")
    tfluids.velocityUpdateForward(U, flags, p)
    p.zero_()
    batch = dict(pDiv=p, UDiv=U, flags=flags, density=density, div=div)
    (ubc, umk), (dbc, dmk) = emitter_pairs(plan)
    if ubc is not None:
        batch["UBC"], batch["UBCInvMask"] = torch.from_numpy(ubc).to(device), torch.from_numpy(umk).to(device)
    if dbc is not None:
        batch["densityBC"], batch["densityBCInvMask"] = torch.from_numpy(dbc).to(device), torch.from_numpy(dmk).to(device)
    return batch


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def saved_steps(gconf):
    return list(range(0, int(gconf["steps"]), int(gconf["saveEvery"])))


def frame_paths(out_dir, prefix, run, frame):
    """<out_dir>/<prefix>/<run %06d>/<frame %06d>[_divergent].bin -- out_dir = <dataDir>/<dataset> of data.scan"""
    d = os.path.join(out_dir, prefix, "%06d" % run)
    return os.path.join(d, "%06d.bin" % frame), os.path.join(d, "%06d_divergent.bin" % frame)


def run_frames(plan, gconf, store, first_slot, device):
    """One run into slots [first_slot, first_slot + frames): per step an outputDiv step and simulate.project, around a saved step
    the two half-puts. -> the number of frames written."""
    batch, mconf = init_state(plan, device), mconf_of(plan)
    every, n = int(gconf["saveEvery"]), 0
    for k in range(int(gconf["steps"])):
        save = k % every == 0
        simulate(None, mconf, batch, None, outputDiv=True)
        if save:
            store.put_device([first_slot + n], dict(pDiv=batch["pDiv"], UDiv=batch["UDiv"], flags=batch["flags"],
                                                    densityDiv=batch["density"]))
        project(None, mconf, batch)
        if save:
            store.put_device([first_slot + n], dict(pTarget=batch["pDiv"], UTarget=batch["UDiv"], densityTarget=batch["density"]))
            n += 1
    return n


def _write_run(store, is3D, dims, first, n, out_dir, prefix, run):
    """the disk sink: every frame pair of the run read back FROM ITS SLOT and written with io.saveMantaFile"""
    C = 3 if is3D else 2
    buf = {k: torch.empty((1, C if k in ("UDiv", "UTarget") else 1) + tuple(dims), device=store.device) for k in _data._OUTPUTS}
    os.makedirs(os.path.dirname(frame_paths(out_dir, prefix, run, 0)[0]), exist_ok=True)
    for f in range(n):
        store.gather([first + f], buf)
        h = {k: v.cpu().numpy() for k, v in buf.items()}
        fn, fn_div = frame_paths(out_dir, prefix, run, f)
        _io.saveMantaFile(fn, h["pTarget"], h["UTarget"], h["flags"], h["densityTarget"])
        _io.saveMantaFile(fn_div, h["pDiv"], h["UDiv"], h["flags"], h["densityDiv"])


# ---- R runs at a time, as the items of one batch ------------------------------------------------------------------
MAX_BATCH_RUNS = 32       # TFL_MAX_ITEMS: the per-item forces travel in the kernel arguments (and 32 slots x 2 halves fit one put)


def schedule_waves(first_run, nruns, batch_runs, run_wave, div_threshold, keep=None):
    """The order in which generate(batch_runs=R) works through its runs; host code, no GPU. A pending list of (run, attempt) starts
    as (first_run + i, 0); a wave is its next <= batch_runs entries; run_wave(wave) -> the max_div of every entry. An entry above
    div_threshold (None: no filter) appends (run, attempt + 1) to the list -- a retried run lands in a later wave -- and after
    MAX_ATTEMPTS the serial generator's error is raised. keep(j, run): called behind its wave for every entry j of it that is kept
    (the disk sink reads the wave's slots before the next wave reuses them).
    -> (runs kept, report, warnings), each in the order the serial generator produces them: by run, then attempt."""
    pending = [(int(first_run) + i, 0) for i in range(int(nruns))]
    report, notes = [], []
    while pending:
        wave, pending = pending[:batch_runs], pending[batch_runs:]
        divs = run_wave(wave)
        assert len(divs) == len(wave)
        for j, ((run, attempt), max_div) in enumerate(zip(wave, divs)):
            kept = div_threshold is None or max_div <= float(div_threshold)
            report.append(dict(run=run, attempt=attempt, max_div=max_div, kept=kept))
            if kept:
                if keep is not None:
                    keep(j, run)
                continue
            if attempt + 1 >= MAX_ATTEMPTS:
                raise TfluidsError("generate: run %d exceeded the divergence threshold %d times" % (run, MAX_ATTEMPTS))
            notes.append((run, attempt, "generated run %d (attempt %d) has max(div) = %g above the threshold %g: generating it again"
                          % (run, attempt, max_div, float(div_threshold))))
            pending.append((run, attempt + 1))
    report.sort(key=lambda r: (r["run"], r["attempt"]))
    return [r["run"] for r in report if r["kept"]], report, [n[2] for n in sorted(notes)]


def join_states(states):
    """B = 1 batches of one shape (init_state) as one [B]-wide batch. A BC pair is the identity (mask 1, value 0) for the items
    without one and is left out where no item has it."""
    batch = {k: torch.cat([st[k] for st in states], 0) for k in ("pDiv", "UDiv", "flags", "density", "div")}
    for bc, mask in (("UBC", "UBCInvMask"), ("densityBC", "densityBCInvMask")):
        if any(bc in st for st in states):
            like = next(st[bc] for st in states if bc in st)
            batch[bc] = torch.cat([st[bc] if bc in st else torch.zeros_like(like) for st in states], 0)
            batch[mask] = torch.cat([st[mask] if mask in st else torch.ones_like(like) for st in states], 0)
    return batch


def init_wave(plans, device):
    """The S_0 of every plan (init_state, one run at a time as in the serial generator: its cost, the host read included, is per
    run) joined into one batch, and the forces of every item. -> (batch, mconf, item_forces); mconf's shared fields (dt, the
    method, the strength, maxIter, pcgPrecond) are equal over the plans by construction."""
    batch = join_states([init_state(p, device) for p in plans])
    mconfs = [mconf_of(p) for p in plans]
    shared = ("dt", "advectionMethod", "maccormackStrength", "simMethod", "maxIter", "pcgPrecond")
    assert all(m[k] == mconfs[0][k] for m in mconfs for k in shared)
    forces = [{k: m[k] for k in ("gravity", "buoyancyScale", "gravityScale", "vorticityConfinementAmp")} for m in mconfs]
    return batch, mconfs[0], forces


def wave_frames(plans, gconf, store, first_slots, device):
    """run_frames for a wave: the runs of `plans` as the items of one batch, item j into slots [first_slots[j], + frames). Per
    step an outputDiv items step and project_items; around a saved step ONE put per half for all items. -> frames written per run."""
    batch, mconf, forces = init_wave(plans, device)
    every, n = int(gconf["saveEvery"]), 0
    for k in range(int(gconf["steps"])):
        save = k % every == 0
        simulate_items(None, mconf, batch, forces, outputDiv=True)
        if save:
            store.put_device([f + n for f in first_slots], dict(pDiv=batch["pDiv"], UDiv=batch["UDiv"], flags=batch["flags"],
                                                                densityDiv=batch["density"]))
        project_items(None, mconf, batch, forces)
        if save:
            store.put_device([f + n for f in first_slots], dict(pTarget=batch["pDiv"], UTarget=batch["UDiv"],
                                                                densityTarget=batch["density"]))
            n += 1
    return n


def _generate_waves(gconf, prefix, nruns, seed, out_dir, store, device, first_run, batch_runs):
    is3D, dims = bool(gconf["is3D"]), tuple(gconf["dims"])
    frames = len(saved_steps(gconf))
    own = store is None
    if own:
        store = _data.FrameStore(device, is3D, *dims, batch_runs * frames, batch_runs * frames)
    elif store.is3D != is3D or tuple(store.dims) != dims or store.capacity < nruns * frames:
        raise TfluidsError("generate: the store (%s, %d slots) does not hold %d runs of %d frames of %s"
                           % (store.dims, store.capacity, nruns, frames, dims))
    firsts = {}

    def run_wave(wave):
        plans = [plan_run(gconf, seed, run, attempt) for run, attempt in wave]
        firsts.clear()
        firsts.update({j: (j if own else run - first_run) * frames for j, (run, _) in enumerate(wave)})
        n = wave_frames(plans, gconf, store, [firsts[j] for j in range(len(wave))], store.device)
        assert n == frames
        return [_data.max_target_divergence(store, is3D, dims, firsts[j], n) for j in range(len(wave))]

    def keep(j, run):
        if out_dir is not None:
            _write_run(store, is3D, dims, firsts[j], frames, out_dir, prefix, run)

    try:
        kept, report, notes = schedule_waves(first_run, nruns, batch_runs, run_wave, gconf.get("divThreshold"), keep)
        for note in notes:
            warnings.warn(note)
        runs = [("%06d" % run, frames) for run in kept]
        dataset = None if own else _data.DataBinary.from_store(store, runs, is3D, dims)
    finally:
        if own:
            store.close()
    return dict(runs=runs, report=report, data=dataset)


def generate(gconf, prefix, nruns, seed, out_dir=None, store=None, device="cuda", first_run=0, batch_runs=1):
    """nruns runs (numbers first_run ...) of gconf's scenes under `seed`, saved_steps(gconf) frame pairs each.
    batch_runs = R > 1 (at most MAX_BATCH_RUNS): R runs are stepped at a time as the items of one batch (schedule_waves,
    wave_frames) -- the same frames in the same slots and files, the same runs and report as one run at a time, which stays the
    default; it pays where a step is launch-bound (profiles/datagen_batched.md). The scratch store then holds R runs.
    store: a data.FrameStore of the right shape with room for nruns * frames records (None with out_dir: a scratch store of ONE
    run is used); run i's frames go to slots [i * frames, (i + 1) * frames), straight from the simulation's tensors.
    out_dir: <dataDir>/<dataset>; the frames are also written as <out_dir>/<prefix>/<run %06d>/<frame %06d>[_divergent].bin.
    A run whose signed maximum target divergence exceeds gconf['divThreshold'] (None: no filter) is generated again with the next
    sub-seed (attempt), at most MAX_ATTEMPTS times; what happened is reported.
    -> {"runs": [(name, frames)], "report": [{run, attempt, max_div, kept}], "data": DataBinary.from_store(...) or None}"""
    if out_dir is None and store is None:
        raise TfluidsError("generate: neither a store nor an out_dir to write to")
    batch_runs = int(batch_runs)
    if batch_runs < 1 or batch_runs > MAX_BATCH_RUNS:
        raise TfluidsError("generate: batch_runs = %d, 1 to %d runs are stepped at a time" % (batch_runs, MAX_BATCH_RUNS))
    if batch_runs > 1:
        return _generate_waves(gconf, prefix, nruns, seed, out_dir, store, device, first_run, batch_runs)
    is3D, dims = bool(gconf["is3D"]), tuple(gconf["dims"])
    frames = len(saved_steps(gconf))
    own = store is None
    if own:
        store = _data.FrameStore(device, is3D, *dims, frames, frames)
    elif store.is3D != is3D or tuple(store.dims) != dims or store.capacity < nruns * frames:
        raise TfluidsError("generate: the store (%s, %d slots) does not hold %d runs of %d frames of %s"
                           % (store.dims, store.capacity, nruns, frames, dims))
    runs, report = [], []
    try:
        for i in range(int(nruns)):
            run, first = first_run + i, 0 if own else i * frames
            for attempt in range(MAX_ATTEMPTS):
                plan = plan_run(gconf, seed, run, attempt)
                n = run_frames(plan, gconf, store, first, store.device)
                max_div = _data.max_target_divergence(store, is3D, dims, first, n)
                kept = gconf.get("divThreshold") is None or max_div <= float(gconf["divThreshold"])
                report.append(dict(run=run, attempt=attempt, max_div=max_div, kept=kept))
                if kept:
                    break
                warnings.warn("generated run %d (attempt %d) has max(div) = %g above the threshold %g: generating it again"
                              % (run, attempt, max_div, float(gconf["divThreshold"])))
            else:
                raise TfluidsError("generate: run %d exceeded the divergence threshold %d times" % (run, MAX_ATTEMPTS))
            if out_dir is not None:
                _write_run(store, is3D, dims, first, n, out_dir, prefix, run)
            runs.append(("%06d" % run, n))
        dataset = None if own else _data.DataBinary.from_store(store, runs, is3D, dims)
    finally:
        if own:
            store.close()
    return dict(runs=runs, report=report, data=dataset)
