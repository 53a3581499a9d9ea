"""rigl.cifar_resnet.data_helper -> rigl_amd.data."""
from rigl_amd.data import (  # noqa: F401
    IMG_SIZE, DeviceCifar, input_fn, load_cifar10_python, pad_input, preprocess_train)
