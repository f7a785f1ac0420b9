"""Drop-in for the reference's Env/benchmarks.py (see Env/market_env.py here):
the same classes, plus ``quote_rule`` to run them on the device."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _sgmm_path import sgmm  # noqa: E402

FOICPolicy = sgmm.FOICPolicy
GLFTPolicy = sgmm.GLFTPolicy
quote_rule = sgmm.quote_rule
