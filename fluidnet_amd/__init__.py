"""fluidnet_amd -- MI355X-native tfluids.simulate() hot path behind FluidNet's tfluids.* API.

  fluidnet_amd.tfluids    host mirror of torch/tfluids/init.lua (operators; ctypes over the C ABI)
  fluidnet_amd.simulate   host mirror of torch/lib/simulate.lua (simulate, setConstVals, createPlumeBCs)
  fluidnet_amd.model      the `default` projection ConvNet (lib/model.lua) over tfl_model_forward
  fluidnet_amd.stats      host mirror of the rollout of torch/lib/calc_stats.lua (calcStats: divergence norm over time)
  fluidnet_amd.train      ProjectionNet: the net as a torch.nn.Module over tfl_model_forward_train / tfl_model_backward
  fluidnet_amd.optim      Adam / RMSprop: gradient clip + lib/adam.lua / lib/rmsprop.lua + weight refresh over tfl_optim_step
  fluidnet_amd.criterion  nn.FluidCriterion (torch/lib/modules/fluid_criterion.lua) over tfl_fluidCriterion
  fluidnet_amd.run_epoch  the training closure of torch/lib/run_epoch.lua (long-term divergence pass included) as one call
  fluidnet_amd.data       torch/lib/data_binary.lua: the data set in a resident frame store (tfl_frames_*), mini-batches by one launch
  fluidnet_amd.datagen    training sets generated on the device: random scenes, PCG frame pairs, into a frame store or onto the disk
  fluidnet_amd.train_loop the loop of torch/fluid_net_train.lua: fit() -- epochs, last / best model files, log, resume
  fluidnet_amd.dist       z-slab decomposition across GPUs: halo exchange + 1 all-reduce per step (RCCL); the transports that
                          data-parallel training (optim.step(comm=...), run_epoch.Closure(comm=...)) reduces its gradients over
  fluidnet_amd.csrc/      hand-written HIP kernels for gfx950 + the C ABI (include/tfluids_hip.h)
"""
from . import tfluids  # noqa: F401
from . import simulate  # noqa: F401  (module: simulate.simulate, .createPlumeBCs, .setConstVals)
from .model import FluidNetModel, load_model  # noqa: F401
from . import stats  # noqa: F401  (module: stats.calcStats)
from . import criterion  # noqa: F401
from .criterion import FluidCriterion  # noqa: F401  (nn.FluidCriterion: loss terms and input gradients in one pass)
from .simulate import calcPUTargets, dataAugmentation  # noqa: F401  (the training targets by a Jacobi / PCG projection; the forces added before it)
from .train import ProjectionNet  # noqa: F401  (the projection net as an nn.Module: forward with a tape, parameter gradients)
from . import optim  # noqa: F401  (optim.Adam / optim.RMSprop: clip + update + weight refresh as one device call)
from . import run_epoch  # noqa: F401  (run_epoch.plan_batch / Closure / run_epoch: one call for a training mini-batch)
from . import dist  # noqa: F401  (transports: DistComm / RcclComm / ThreadComm; the z-slab step; run_virtual_closures)
from . import data  # noqa: F401  (data.DataBinary: the training set in a resident frame store, one launch per mini-batch)
from . import datagen  # noqa: F401  (datagen.plan_run / init_state / generate: the producer of what fit() reads)
from . import train_loop  # noqa: F401  (train_loop.fit: epochs, best / last model files, log, resume)
from . import modules  # noqa: F401  (the tfluids nn.Modules as torch.nn.Modules with autograd)
from ._lib import TfluidsError  # noqa: F401
