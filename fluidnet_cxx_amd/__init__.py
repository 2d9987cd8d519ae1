"""fluidnet_cxx_amd: MI355X-native fluid time-step behind fluidnet_cxx's operator surface.

    from fluidnet_cxx_amd import fluid, simulate, FluidNet     # mirrors the reference's `lib`
    from fluidnet_cxx_amd import FluidNetTrain                 # the same net with a native backward pass (2D)
    from fluidnet_cxx_amd import FluidNetBankTrain             # ... for the 16-channel bank net, mconf['model'] = 'FluidNet' (2D)
    from fluidnet_cxx_amd import FluidNetTrain3D               # ... and its Conv3d counterpart (3D grids)
    from fluidnet_cxx_amd import FluidNetBankTrain3D           # ... and the Conv3d bank net, mconf['model'] = 'FluidNet3D'
    from fluidnet_cxx_amd.training import train, SceneSampler  # the training loop on scenes generated on the device (2D)
    from fluidnet_cxx_amd.training3d import train3d, SceneSampler3D   # ... and in 3D

Importing the operator modules loads the native extension; there is no CPU fallback.
"""


def __getattr__(name):
    import importlib
    if name == "fluid":
        return importlib.import_module(".fluid", __name__)
    if name == "simulate":
        return importlib.import_module("._simulate", __name__).simulate
    if name in ("save_restart", "load_restart", "rollout"):
        return getattr(importlib.import_module(".state_io", __name__), name)
    if name == "output":
        return importlib.import_module(".output", __name__)
    if name in ("FluidNet", "MultiScaleNet", "BankNet", "BankNet3D"):
        return getattr(importlib.import_module(".model", __name__), name)
    if name == "FluidNetTrain":
        return importlib.import_module(".train", __name__).FluidNetTrain
    if name == "FluidNetBankTrain":
        return importlib.import_module(".train", __name__).FluidNetBankTrain
    if name == "FluidNetBankTrain3D":
        return importlib.import_module(".train", __name__).FluidNetBankTrain3D
    if name == "FluidNetTrain3D":
        return importlib.import_module(".train3d", __name__).FluidNetTrain3D
    raise AttributeError(name)
