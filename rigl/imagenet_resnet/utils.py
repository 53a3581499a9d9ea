"""rigl.imagenet_resnet.utils -> rigl_amd.summaries."""
from rigl_amd.summaries import mask_summaries  # noqa: F401
