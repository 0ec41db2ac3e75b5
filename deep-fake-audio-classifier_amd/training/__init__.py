"""Training-side pieces: checkpoint format (counterpart of src/training/checkpoint.py) and, in train_step.py, the
train-mode forward/backward path."""
from .checkpoint import build_config_dict, checkpoint_blob, load_checkpoint, save_checkpoint  # noqa: F401


def cnn2d_train_forward(model, x, return_embedding=False):
    from .train_step import cnn2d_train_forward as _impl
    return _impl(model, x, return_embedding)


def cnn1d_train_forward(model, x):
    from .train_step import cnn1d_train_forward as _impl
    return _impl(model, x)


def cae_train_forward(model, x):
    from .train_step import cae_train_forward as _impl
    return _impl(model, x)


def __getattr__(name):
    if name == "DlqTrainer":        # the DeepfakeDetector's all-C-ABI trainer (train_step.py), imported on first use
        from .train_step import DlqTrainer
        return DlqTrainer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
