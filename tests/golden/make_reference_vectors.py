"""Regenerate the recorded results of the reference implementation that the CPU tests compare to.

    python tests/golden/make_reference_vectors.py --reference <checkout of the reference project>

The reference's ``neural_net_model.py`` is loaded from the given directory, run on the scenarios
below (the same seeds and arguments the tests use), and what it computed / wrote is stored here:

* ``reference_train_9_18_9.json`` — parameters after initialisation and after ``train()``, the
  per-epoch costs and weight update ratios, the average cost and the stats
  (``test_init_and_training_bit_identical_to_reference``);
* ``reference_ckpt/model_x.json`` + ``reference_ckpt/optimizer_x.pth`` — a checkpoint exactly as
  the reference's ``serialize()`` writes it (``test_reference_checkpoints_interoperate``).

Only data is stored; no source of the reference is copied.
"""
import argparse
import importlib.util
import json
import os
import shutil
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

TRAIN_ARGS = ([9, 18, 9], "xavier", "random", ["relu", "softmax"], "adam")


def train_data(n: int) -> list:
    return [([float((i * 7 + j) % 5 - 2) for j in range(9)], [i % 9]) for i in range(n)]


def _load(reference_dir: str):
    spec = importlib.util.spec_from_file_location("ref_neural_net_model",
                                                  os.path.join(reference_dir, "neural_net_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="directory holding the reference's neural_net_model.py")
    args = ap.parse_args()
    ref = _load(os.path.abspath(args.reference))
    cwd = os.getcwd()
    work = tempfile.mkdtemp(prefix="pz_golden_")
    os.chdir(work)  # the reference writes models/ under the current directory
    try:
        torch.manual_seed(42)
        r = ref.NeuralNetworkModel("r", *TRAIN_ARGS)
        init = [p.tolist() for p in r.params]
        torch.manual_seed(7)
        r.train(train_data(r.training_buffer_size), epochs=3, batch_size=32)
        with open(os.path.join(HERE, "reference_train_9_18_9.json"), "w") as f:
            json.dump({"torch": torch.__version__,
                       "init_params": init,
                       "trained_params": [p.tolist() for p in r.params],
                       "costs": [p["cost"] for p in r.progress],
                       "weight_upd_ratio": [p["weight_upd_ratio"] for p in r.progress],
                       "avg_cost": r.avg_cost,
                       "stats": r.stats}, f, indent=1)

        torch.manual_seed(3)
        x = ref.NeuralNetworkModel("x", [8, 16, 4], activation_algos=["tanh", "softmax"], optimizer_algo="adam")
        x.serialize()
        out = os.path.join(HERE, "reference_ckpt")
        os.makedirs(out, exist_ok=True)
        for name in ("model_x.json", "optimizer_x.pth"):
            shutil.copyfile(os.path.join(work, "models", name), os.path.join(out, name))
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
