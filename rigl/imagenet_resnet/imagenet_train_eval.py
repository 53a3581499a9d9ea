"""rigl.imagenet_resnet.imagenet_train_eval (set_lr_schedule + lr_schedule, :280-330) -> rigl_amd.schedules."""
from rigl_amd.schedules import imagenet_lr_schedule  # noqa: F401
