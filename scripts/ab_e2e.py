"""Same-session A/B of the tools that scripts/sample_e2e.py, uniq_e2e.py or sort_e2e.py time: this build against another one's.

The named script's own main() runs once -- one generated input, its own cases and --reps -- but every timed command that starts a
tool which also exists in the other build's bin directory is run alternately from there and from highperformancengs_amd/bin
(other, this / this, other / ...; the last run is this build's, so the script's own JSON, written to --out as ever, holds this
build's walls).  <ab-out> receives both sets of walls per case, whether this build's median lies within the other's spread
(min to max), and whether the two builds' last runs wrote outputs of the same size and SHA-256 -> profiles/feed/*_ab.json.

    python scripts/ab_e2e.py sample|uniq|sort <other build's bin directory> <ab-out .json> [arguments of the script]
"""
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    tool, other, ab_out = sys.argv[1], os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])
    mod = importlib.import_module(tool + "_e2e")
    timed_once, digest_dir = mod.timed, mod.digest_dir
    cases = []

    def timed(cmd, cwd, env=None, reps=1):
        exe = os.path.basename(cmd[0])
        if os.path.dirname(cmd[0]) != mod.BIN or not os.path.exists(os.path.join(other, exe)):
            return timed_once(cmd, cwd, env, reps)
        walls, digests, err = {"other": [], "this": []}, {}, ""
        for rep in range(reps):
            for who in (["other", "this"] if (reps - 1 - rep) % 2 == 0 else ["this", "other"]):
                w, e = timed_once([os.path.join(other if who == "other" else mod.BIN, exe)] + cmd[1:], cwd, env, 1)
                walls[who] += w
                if who == "this":
                    err = e
                if rep == reps - 1:
                    digests[who] = digest_dir(cwd)
        o, t = walls["other"], walls["this"]
        cases.append({"cmd": [exe] + [os.path.basename(x) if x.startswith("/") else x for x in cmd[1:]], "other_wall_s": o, "this_wall_s": t,
                      "this_median_s": statistics.median(t), "within_other_spread": min(o) <= statistics.median(t) <= max(o),
                      "same_outputs": digests["other"] == digests["this"]})
        print("AB", json.dumps(cases[-1]), flush=True)
        os.makedirs(os.path.dirname(ab_out), exist_ok=True)
        with open(ab_out, "w") as f:
            json.dump({"script": "scripts/%s_e2e.py" % tool, "cases": cases}, f, indent=1)
            f.write("\n")
        return t, err

    mod.timed = timed
    sys.argv = ["scripts/%s_e2e.py" % tool] + sys.argv[4:]
    mod.main()


if __name__ == "__main__":
    main()
