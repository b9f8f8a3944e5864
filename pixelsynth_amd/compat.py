"""Make the reference's import paths resolve to the MI355X implementation (option A), so
drivers written against crockwell/pixelsynth (`demo.py`, `create_vid.py`, `evaluation/*.py`) pick up the HIP
path without source edits:

    import pixelsynth_amd.compat; pixelsynth_amd.compat.install_reference_aliases()

The reference's metric modules (`evaluation.metrics`, `models.losses.ssim`) are aliased separately, by install_evaluation_aliases().
"""
import importlib
import importlib.util
import sys
import types

ALIASES = {
    "models.projection.z_buffer_manipulator": "pixelsynth_amd.projection.z_buffer_manipulator",
    "models.layers.z_buffer_layers": "pixelsynth_amd.layers.z_buffer_layers",
    "models.lmconv.locally_masked_convolution": "pixelsynth_amd.lmconv.locally_masked_convolution",
    "models.lmconv.layers": "pixelsynth_amd.lmconv.layers",
    "models.lmconv.model": "pixelsynth_amd.lmconv.model",
    "models.lmconv.masking": "pixelsynth_amd.lmconv.masking",
    "models.lmconv.sample": "pixelsynth_amd.lmconv.sample",
    "models.lmconv.utils": "pixelsynth_amd.lmconv.utils",
    "models.vqvae2.vqvae": "pixelsynth_amd.vqvae2.vqvae",
}


def _parent_package(pkg):
    """The reference's own package when its tree is importable (demo.py run from a checkout: everything that is NOT
    aliased -- models.networks, models.base_model, ... -- must keep resolving through the real package's __path__);
    an empty namespace module only when there is nothing to import."""
    if pkg in sys.modules:
        return sys.modules[pkg]
    try:
        return importlib.import_module(pkg)
    except Exception:   # ImportError, or a package __init__ that needs what this machine lacks
        sys.modules.pop(pkg, None)
    m = types.ModuleType(pkg)
    m.__path__ = []
    spec = None
    try:
        spec = importlib.util.find_spec(pkg)
    except Exception:
        pass
    if spec is not None and spec.submodule_search_locations:
        m.__path__ = list(spec.submodule_search_locations)   # the real directory: non-aliased submodules still resolve
    sys.modules[pkg] = m
    return m


def install_reference_aliases(force=False):
    """Register the mirrors under the reference's module names."""
    installed = []
    for ref, ours in ALIASES.items():
        if ref in sys.modules and not force:
            continue
        parts = ref.split(".")
        for i in range(1, len(parts)):
            pkg = ".".join(parts[:i])
            parent = _parent_package(pkg)
            if i > 1:
                setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], parent)
        mod = importlib.import_module(ours)
        sys.modules[ref] = mod
        setattr(sys.modules[".".join(parts[:-1])], parts[-1], mod)
        installed.append(ref)
    return installed


EVAL_ALIASES = {
    "evaluation.metrics": "pixelsynth_amd.evaluation.metrics",
    "models.losses.ssim": "pixelsynth_amd.losses.ssim",
}


def install_evaluation_aliases(force=False):
    """Register the metric mirrors (PSNR / SSIM on the HIP kernel) under the reference's module names, so its scoring scripts
    (`from evaluation.metrics import psnr, ssim_metric`) run unchanged.  Separate from install_reference_aliases: it claims the
    reference's `evaluation` package name."""
    installed = []
    for ref, ours in EVAL_ALIASES.items():
        if ref in sys.modules and not force:
            continue
        parts = ref.split(".")
        for i in range(1, len(parts)):
            pkg = ".".join(parts[:i])
            parent = _parent_package(pkg)
            if i > 1:
                setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], parent)
        mod = importlib.import_module(ours)
        sys.modules[ref] = mod
        setattr(sys.modules[".".join(parts[:-1])], parts[-1], mod)
        installed.append(ref)
    return installed


TRAINING_ALIASES = {
    "models.losses.synthesis": "pixelsynth_amd.losses.synthesis",
}


def _install(table, force):
    """Register the mirrors of `table` under the reference's module names -> the names installed"""
    installed = []
    for ref, ours in table.items():
        if ref in sys.modules and not force:
            continue
        parts = ref.split(".")
        for i in range(1, len(parts)):
            parent = _parent_package(".".join(parts[:i]))
            if i > 1:
                setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], parent)
        mod = importlib.import_module(ours)
        sys.modules[ref] = mod
        setattr(sys.modules[".".join(parts[:-1])], parts[-1], mod)
        installed.append(ref)
    return installed


def install_training_aliases(force=False):
    """Register the generator's image loss (SynthesisLoss and its terms, the VGG19 content term on the HIP kernels) under the
    reference's module name, so a training script's `from models.losses.synthesis import SynthesisLoss` runs unchanged.  Separate
    from the other two: a caller that only renders or scores does not import the loss."""
    return _install(TRAINING_ALIASES, force)


GAN_ALIASES = {
    "models.losses.gan_loss": "pixelsynth_amd.losses.gan_loss",
    "models.networks.discriminators": "pixelsynth_amd.networks.discriminators",
}


def install_gan_aliases(force=False):
    """Register the discriminator and its losses (DiscriminatorLoss with both one-step entry points, the instance norm and the feature
    matching on the HIP kernels when training) under the reference's module names, so `from models.losses.gan_loss import
    DiscriminatorLoss` in models/base_model.py runs unchanged.  A table of its own: a caller picks the adversarial half by itself."""
    return _install(GAN_ALIASES, force)


BASE_MODEL_ALIASES = {
    "models.base_model": "pixelsynth_amd.base_model",
}


def install_base_model_aliases(force=False):
    """Register the training step (BaseModel: the model, the discriminator, both optimisers, one step per call) under the reference's
    module name, so a training script's `from models.base_model import BaseModel` runs unchanged.  A table of its own: the other
    install_* functions register what they registered before, and a caller that keeps the reference's own step does not call this."""
    return _install(BASE_MODEL_ALIASES, force)
