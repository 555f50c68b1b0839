#!/usr/bin/env python3
"""Module-level constants of the reference's training drivers (run where a
checkout of the reference is at hand; it does not travel with the tests):

    python tests/golden/gen_driver_constants.py --ref <reference checkout>

Reads each driver as text (never imports it) and writes the literal settings
(MODEL_PARAMS, the N list's bounds, episodes, MAX_STEPS, epsilon range, paths) to
tests/golden/ref_driver_constants.json, which tests/test_train.py compares
ffm_amd/train.py's DRIVERS against.
"""
from __future__ import annotations

import argparse
import ast
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = ("run_actor_only_training.py", "run_critic_training.py", "run_unified_actor_training.py",
           "run_unified_critic_training.py")


def constants(path):
    tree = ast.parse(open(path, encoding="utf-8").read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            try:
                out[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                if isinstance(node.value, ast.Dict):      # MODEL_PARAMS references EPSILON_START
                    d = {}
                    for k, v in zip(node.value.keys, node.value.values):
                        d[ast.literal_eval(k)] = (out[v.id] if isinstance(v, ast.Name) else ast.literal_eval(v))
                    out[node.targets[0].id] = d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (SoraKurihara/FFM)")
    args = ap.parse_args()
    res = {s: constants(os.path.join(args.ref, s)) for s in SCRIPTS}
    with open(os.path.join(HERE, "ref_driver_constants.json"), "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
