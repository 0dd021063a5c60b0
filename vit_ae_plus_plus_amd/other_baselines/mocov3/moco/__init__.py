"""``builder`` (MoCo, MoCo_ViT) and ``optimizer`` (LARS) under the reference's module names."""
from . import builder, optimizer  # noqa: F401
