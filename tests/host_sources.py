"""Where the tests that read the host sources find what they look for: one file each, so that a
tuning key or a constant that moves to another file fails the test that pins it."""
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "rust_gpu_raytracing_amd" / "csrc"

TUNING = CSRC / "rt_abi.cpp"      # defines rt_set_tuning
CONTEXT = CSRC / "rt_ctx.h"       # struct rt_ctx and the defaults of its tuning fields (kDefault*Chunk)
