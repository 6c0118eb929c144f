"""The on-disk form of a training checkpoint (TrainPipeline.save_checkpoint / resume=): a directory of JSON and .npy files.

  state.json               the pipeline's own values (format version, the configuration keys a resumed run must share,
                           schedule, counters, histories) -- written by rank 0
  <part>.json              the plain values of one part ("meta") and the names of its arrays
  <part>.<array>.npy       one array each, written and read without pickling
  COMPLETE                 empty; written last

Parts: selfplay_rank<r> (SelfPlayEngine.state() of rank r), trainer (HipTrainer.state()), buffer (the replay buffer's
state()), weights (the evaluator's parameters, where no trainer exists yet).  A part's .json is written after its arrays and
moved into place in one step, so a part that can be read is whole.  The directory is filled under `<path>.tmp` and renamed
to `<path>` once COMPLETE is in it; a directory without COMPLETE is not a checkpoint.  Python's json writes float64 values
with repr (they read back bit for bit) and NaN as NaN.
"""
import json
import os
import shutil

import numpy as np

FORMAT = 1


def tmp_path(path):
    return path.rstrip("/") + ".tmp"


def _write_json(path, obj):
    with open(path + ".part", "w") as f:
        json.dump(obj, f)
    os.replace(path + ".part", path)


def begin(path):
    """An empty `<path>.tmp` (a left-over one of an interrupted save is dropped) -> its name"""
    tmp = tmp_path(path)
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)
    os.makedirs(tmp)
    return tmp


def write_part(directory, part, state):
    """state: {"meta": plain values, name: ndarray, ...} (the form every state() of this package returns) -> bytes written"""
    names = sorted(k for k in state if k != "meta")
    total = 0
    for k in names:
        fn = os.path.join(directory, "%s.%s.npy" % (part, k.replace("/", ".")))
        np.save(fn, np.asarray(state[k]), allow_pickle=False)
        total += os.path.getsize(fn)
    _write_json(os.path.join(directory, part + ".json"), {"meta": state.get("meta", {}), "arrays": names})
    return total


def has_part(directory, part):
    return os.path.exists(os.path.join(directory, part + ".json"))


def read_part(directory, part):
    with open(os.path.join(directory, part + ".json")) as f:
        head = json.load(f)
    out = {"meta": head["meta"]}
    for k in head["arrays"]:
        out[k] = np.load(os.path.join(directory, "%s.%s.npy" % (part, k.replace("/", "."))), allow_pickle=False)
    return out


def finish(path, state):
    """state.json, COMPLETE, then `<path>.tmp` becomes `<path>` (an older checkpoint of that name is replaced)"""
    tmp = tmp_path(path)
    _write_json(os.path.join(tmp, "state.json"), state)
    with open(os.path.join(tmp, "COMPLETE"), "w"):
        pass
    if os.path.isdir(path):
        shutil.rmtree(path)
    os.rename(tmp, path)


def read_state(path):
    """-> state.json of a complete checkpoint; ValueError for a directory without COMPLETE or of another format"""
    if not os.path.isdir(path) or not os.path.exists(os.path.join(path, "COMPLETE")):
        raise ValueError("%s is not a complete checkpoint (no COMPLETE file: the save that wrote it did not finish)" % path)
    with open(os.path.join(path, "state.json")) as f:
        state = json.load(f)
    if state.get("format") != FORMAT:
        raise ValueError("%s has checkpoint format %r, this code reads format %r" % (path, state.get("format"), FORMAT))
    return state


def complete_checkpoints(directory, prefix="ckpt_"):
    """The complete checkpoints under `directory` whose names start with `prefix`, oldest first (names sort by batch)"""
    if not os.path.isdir(directory):
        return []
    return [os.path.join(directory, d) for d in sorted(os.listdir(directory))
            if d.startswith(prefix) and not d.endswith(".tmp") and os.path.exists(os.path.join(directory, d, "COMPLETE"))]


def prune(directory, keep, prefix="ckpt_"):
    """Remove all but the newest `keep` complete checkpoints"""
    done = complete_checkpoints(directory, prefix)
    for old in done[:max(0, len(done) - max(1, int(keep)))]:
        shutil.rmtree(old, ignore_errors=True)


def rng_to_json(rng):
    version, key, gauss = rng.getstate()
    return [version, list(key), gauss]


def rng_from_json(rng, value):
    rng.setstate((int(value[0]), tuple(int(x) for x in value[1]), value[2]))
