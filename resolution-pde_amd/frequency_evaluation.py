#!/usr/bin/env python3
"""Error by frequency of trained checkpoints (reference: frequency_evaluation.py, without the plots):
`python frequency_evaluation.py model=ffno_2d/ffno_2d dataset=synthetic/ns_256 checkpoint_dir=...` prints one JSON
document {models: {checkpoint: {resolution: {error, solution, frequencies}}}}."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rpde.entry import run_frequency  # noqa: E402

if __name__ == "__main__":
    run_frequency()
