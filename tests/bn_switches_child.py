"""Child process of tests/test_bn_switches_gpu.py: the whole-network gates of tests/test_model_gpu.py, called unchanged, under the
environment the parent set -- VPD_FUSED_BN=0, the separate finalize / apply / reduce launches.  The switch is read once per process,
so this needs a fresh interpreter.
usage: bn_switches_child.py gates
The gates: test_backward_in_a_well_conditioned_regime for resnet18 and resnet50, test_student_matches_reference_and_oracle on
r18_c5_d32_m1_n8.npz (loss, gradients, the three-step trajectory and the running statistics against the golden file); then every
engine the gates built reports no barrier time-out.  The first failure ends the run: nothing is started after it.
Prints "RESULT <json>": {"fused_bn", "ran": [...], "fail": [...], "engines", "sync_errors"}."""
import json
import os
import sys
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main():
    assert sys.argv[1:] == ["gates"], __doc__
    from tests import test_model_gpu as G
    from vpd_amd import engine as E
    # the gates' record of the default path (parity_*.json under test_model_gpu.OUT) is not this run's to overwrite
    G.OUT = os.path.join(G.OUT, "fused_bn_%s" % os.environ.get("VPD_FUSED_BN", "default"))
    engines = []
    init = E.StudentEngine.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        engines.append(self)
    E.StudentEngine.__init__ = recording_init
    gates = [("well_conditioned/resnet18", lambda: G.test_backward_in_a_well_conditioned_regime("resnet18")),
             ("well_conditioned/resnet50", lambda: G.test_backward_in_a_well_conditioned_regime("resnet50")),
             ("student/r18_c5_d32_m1_n8", lambda: G.test_student_matches_reference_and_oracle(os.path.join(G.GOLDEN, "r18_c5_d32_m1_n8.npz")))]
    out = {"fused_bn": os.environ.get("VPD_FUSED_BN"), "ran": [], "fail": [], "engines": 0, "sync_errors": None}
    for name, gate in gates:
        try:
            gate()
            out["ran"].append(name)
        except BaseException:      # (an assertion of the gate, or an error of the library: either way nothing more is started)
            out["fail"].append("%s: %s" % (name, traceback.format_exc()[-1500:]))
            break
    if not out["fail"]:
        out["engines"] = len(engines)
        out["sync_errors"] = sum(e.sync_errors() for e in engines)
    print("RESULT " + json.dumps(out))
    return 1 if out["fail"] else 0


if __name__ == "__main__":
    sys.exit(main())
