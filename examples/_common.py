import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402,F401
import __graft_entry__ as entry  # noqa: E402

nhp = entry.load_package()


def show(title, truth, estimate):
    print(title)
    print(np.column_stack([truth, estimate])[:12])


def discrete_data(process, duration, seed, device_rand=False):
    """The data of a discrete example: the host simulator, or with --device-rand the GPU generator (disc_rand)."""
    if device_rand:
        return nhp.disc_rand(process, duration, seed=seed)
    return nhp.synthetic.rand(process, duration, seed=seed)


def device_rand_switch():
    return "--device-rand" in sys.argv[1:]
