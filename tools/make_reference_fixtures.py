#!/usr/bin/env python3
"""Copy the reference data that tests/test_assets.py pins the model tables to into tests/golden/reference/, so that the tests run from the
repository alone:

    python tools/make_reference_fixtures.py <reference checkout>/human_robot_gym

  * settings and scene files, verbatim, under the same relative paths: the MJCF of the robot, the human and the nail, the environment
    yamls with every file their defaults lists compose, the wrapper yamls, failsafe.json, schunk.json, the ICRA-2024 `<task>-SAC.yaml` configs
  * mesh_vertices.npz: the vertex set of every STL mesh the robot and human MJCF use (what compile_model.load_stl reads of a mesh), float32
    as stored in the STL, keyed by the mesh's path relative to models/assets
  * extracted.json: values read from the reference's program text, recorded as data (the file itself is not copied): the measured joints of
    models/objects/human/human.py, the `__init__` keyword defaults of each environment class, the (task, horizon) runs of
    training/icra_2024_run_experiments.sh
"""
import ast
import json
import os
import re
import shutil
import sys
import xml.etree.ElementTree as ET

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import compile_model  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference")

ENV_YAMLS = ["reach_human", "pick_place_human_cart", "pick_place_pointing_human_cart", "human_object_inspection_cart", "human_robot_handover_cart",
             "robot_human_handover_cart", "collaborative_lifting_cart", "collaborative_stacking_cart", "collaborative_hammering_cart"]
ENV_SOURCES = ["reach_human_env.py", "pick_place_human_cartesian_env.py", "pick_place_pointing_human_cartesian_env.py", "human_object_inspection_cartesian_env.py",
               "human_robot_handover_cartesian_env.py", "robot_human_handover_cartesian_env.py", "collaborative_lifting_cartesian_env.py",
               "collaborative_stacking_cartesian_env.py", "collaborative_hammering_cartesian_env.py"]
SETTINGS = ["controllers/failsafe_controller/config/failsafe.json", "models/robots/config/schunk.json",
            "training/config/wrappers/ik_position_delta/default_ik_position_delta.yaml",
            "training/config/wrappers/collision_prevention/default_collision_prevention.yaml",
            "models/assets/robots/schunk/robot.xml", "models/assets/human/human.xml", "models/assets/objects/nail.xml"]
# ReachHumanCart (tests/test_reach_cart.py): the task's environment, expert and state-based wrapper yamls with what their defaults lists compose, and its
# data-collection config (the top-level file alone: its robot / wrappers / run groups are the other fixtures' and the test's own)
REACH_CART_YAMLS = ["training/config/environment/reach_human_cart.yaml", "training/config/expert/reach_human_cart.yaml",
                    "training/config/wrappers/state_based_expert_imitation_reward/reach_human_cart_state_based_expert_imitation_reward.yaml"]
REACH_CART_FILES = ["training/config/reach_human_cart_expert_data_collection.yaml"]
ICRA_SHORT = ["R", "PP", "CL", "RHH", "HRH", "CS"]


def composed_files(path):
    """The yaml and every file its Hydra defaults list pulls in (the composition tests/test_assets.py performs)."""
    import yaml
    d = yaml.safe_load(open(path)) or {}
    out = [path]
    for ent in d.get("defaults", []):
        if ent != "_self_":
            out += composed_files(os.path.join(os.path.dirname(path), ent.split("@")[0] + ".yaml"))
    return out


def constructor_defaults(path):
    """keyword -> default of the first class's __init__ in a source file, from its syntax tree (the file is parsed as text, never imported)"""
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.ClassDef):
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name == "__init__":
                    args, defs, out = f.args.args[1:], f.args.defaults, {}
                    for a, dv in zip(args[len(args) - len(defs):], defs):
                        try:
                            v = ast.literal_eval(dv)
                            out[a.arg] = list(v) if isinstance(v, tuple) else v
                        except ValueError:
                            pass
                    return out
    return {}


def mesh_files(assets):
    """Relative paths (to models/assets) of the meshes compile_model reads: every mesh of robot.xml and human.xml."""
    out = []
    for sub, xml in (("robots/schunk", "robot.xml"), ("human", "human.xml")):
        root = ET.parse(os.path.join(assets, sub, xml)).getroot()
        out += [f"{sub}/{m.get('file')}" for m in root.find("asset").findall("mesh")]
    return sorted(set(out))


def main():
    ref = os.path.abspath(sys.argv[1])
    files = list(SETTINGS)
    env_dir = os.path.join(ref, "training", "config", "environment")
    for name in ENV_YAMLS:
        files += [os.path.relpath(p, ref) for p in composed_files(os.path.join(env_dir, name + ".yaml"))]
    files.append("training/config/environment/default/collaborative_hammering_cart.yaml")
    for rel in REACH_CART_YAMLS:
        files += [os.path.relpath(p, ref) for p in composed_files(os.path.join(ref, rel))]
    files += REACH_CART_FILES
    files += [f"training/config_icra_2024/environment_evaluation/training/{s}-SAC.yaml" for s in ICRA_SHORT]
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    for rel in sorted(set(os.path.normpath(f) for f in files)):
        os.makedirs(os.path.dirname(os.path.join(OUT, rel)), exist_ok=True)
        shutil.copyfile(os.path.join(ref, rel), os.path.join(OUT, rel))

    assets = os.path.join(ref, "models", "assets")
    verts = {}
    for rel in mesh_files(assets):
        V = compile_model.load_stl(os.path.join(assets, rel))
        v32 = V.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), V), rel
        verts[rel] = v32
    np.savez_compressed(os.path.join(OUT, "mesh_vertices.npz"), **verts)

    src = open(os.path.join(ref, "models", "objects", "human", "human.py")).read()
    blk = src[src.index("joint_elements"):]
    runs = re.findall(r"icra_2024_environment_evaluation\.sh (\w+) \w+ \d+ \d+ (\d+) ", open(os.path.join(ref, "training", "icra_2024_run_experiments.sh")).read())
    extracted = {
        "human_joint_elements": re.findall(r'"([A-Za-z_]+)"', blk[:blk.index("]")]),
        "constructor_defaults": {f: constructor_defaults(os.path.join(ref, "environments", "manipulation", f)) for f in ENV_SOURCES},
        "icra_2024_runs": [[s, int(hz)] for s, hz in runs],
    }
    with open(os.path.join(OUT, "extracted.json"), "w") as f:
        json.dump(extracted, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(set(files))} files, {len(verts)} meshes")


if __name__ == "__main__":
    main()
