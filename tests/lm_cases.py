"""The cases that steer the bundle adjustment's Levenberg-Marquardt control (lm_decide_logic / lm_post_logic of
csrc/ba_kernels.h, run by the fused tails, by ba_lm_decide_kernel / ba_lm_post_kernel and by the one-workgroup form)
onto every branch that options alone can reach, and what the oracle (oracle/ba_oracle.c, oracle_ba_solve_trace) makes of
each: tests/test_lm_cases_cpu.py holds the oracle to EXPECT and to the margins below without a device,
tests/test_lm_control_gpu.py holds the device to the oracle.

Scenes (synth.make_ba_scene):
  A      quaternion, 3 cameras x 60 tracks of length 3: the general form with one block (N = 32, small lists, the decide
         kernel clears S, the eager host loop); in the one-workgroup form this is B
  A_far  A started 90 degrees and 0.1 away: a natural mix of accepted and rejected steps (scenarios 11-13; what became
         of the radius 1e16 of 12 and 13: DECIDED_BY_THE_LAST_BITS below)
  C      Euler, 12 cameras x 300 tracks: N = 64; with the decide and post kernels launched on their own this is D
  E      quaternion, 40 cameras x 600 tracks: 195 unknowns, N = 224, so the waiting host loop
  F      quaternion, ring of 200 cameras x 2000 tracks: the elimination order is chosen
  NORMS  Euler, 6 cameras with three free angles each, one camera constant beside camera 0, points constant: which
         coordinates count in |x| and |dx|

SCENARIOS: number -> (scene variant or None, options).  EXPECT: (scene, number) -> (termination, iterations, successful
steps, unsuccessful steps) of the oracle; the GPU test runs exactly the keys of EXPECT.

Margins (margins()): every comparison the oracle made on the way, as (iteration, name, relative distance of the
compared value from its threshold).  A solve whose every margin is at least MARGIN cannot take another branch on the
device unless the device's value is wrong by 1e-3; the two sides agree to 1e-9 .. 1e-11.  The validity test compares the
model cost change with zero, where no relative distance exists.  The model cost change is a sum of terms whose
magnitudes add up to at most 2 sqrt(model_cost_change x_cost) (_terms()), and the two sides agree to 1e-11 of that; its
margin is |model_cost_change| / (1e-5 _terms), so that MARGIN there means 1e-8 of the terms' magnitude: three decades
above what the two sides agree to, as for the other tests.

Brackets (BRACKETS, bracket_options()): the value the oracle compared with a threshold at iteration k becomes that
threshold times (1 +- BRACKET): the solve must take the branch on one side and not on the other, so the device's value
is pinned to 1e-6 -- three decades of room above the agreement of the two sides, and far below what a wrong or missing
term in a norm or a sum moves it by.
"""
import numpy as np

import oracle_lib
from orthosfm_amd import synth

FUNCTION, GRADIENT, PARAMETER, TRUST_REGION, NO_CONVERGENCE, FAILURE = 1, 2, 3, 4, 5, 6
TERM_NAMES = {1: "FUNCTION", 2: "GRADIENT", 3: "PARAMETER", 4: "TRUST_REGION", 5: "NO_CONVERGENCE", 6: "FAILURE"}
MARGIN = 1e-3
BRACKET = 1e-6
DEFAULTS = {"function_tolerance": 1e-6, "gradient_tolerance": 1e-10, "parameter_tolerance": 1e-10, "max_num_iterations": 100,
            "min_trust_region_radius": 1e-32, "min_relative_decrease": 1e-3, "max_consecutive_invalid_steps": 5}

_scenes = {}


def scene(name):
    """A fresh copy of the named scene (built once)."""
    if name not in _scenes:
        if name == "A":
            sc = synth.make_ba_scene(0, 3, 60, config_id=85, min_len=3, max_len=3)
        elif name == "A_far":
            sc = synth.make_ba_scene(0, 3, 60, config_id=85, min_len=3, max_len=3, rot_perturb_deg=90, point_perturb=0.1)
        elif name == "A_nan":
            sc = scene("A")
            sc.obs_xy[47, 1] = np.nan
        elif name == "C":
            sc = synth.make_ba_scene(1, 12, 300, config_id=85)
        elif name == "E":
            sc = synth.make_ba_scene(0, 40, 600, config_id=85)
        elif name == "F":
            sc = synth.make_ba_scene(0, 200, 2000, config_id=81, max_len=12)
        elif name == "NORMS":
            sc = synth.make_ba_scene(1, 6, 150, config_id=85, euler_free=3)
            sc.cam_const[3, :] = 1
        else:
            raise KeyError(name)
        _scenes[name] = sc
    return _scenes[name].copy()


NEGATIVE_DIAGONAL = {"min_lm_diagonal": -1e30, "max_lm_diagonal": -1e30}
SCENARIOS = {
    "1": (None, {}),
    "2": (None, {"gradient_tolerance": 1e30}),
    "3A": (None, {"gradient_tolerance": 50.0}),
    "3C": (None, {"gradient_tolerance": 500.0}),
    "4": (None, {"parameter_tolerance": 1e-4}),
    "5/0": (None, {"max_num_iterations": 0}),
    "5/1": (None, {"max_num_iterations": 1}),
    "5/3": (None, {"max_num_iterations": 3}),
    "6": (None, {"min_trust_region_radius": 1e5}),
    "7": (None, {"min_relative_decrease": 1e3, "max_num_iterations": 6}),
    "8": (None, {"min_relative_decrease": 1e3}),
    "9": (None, {"min_relative_decrease": 1.5}),
    "10": (None, {"min_relative_decrease": 1.5, "min_trust_region_radius": 100.0}),
    "11": ("A_far", {}),
    "12": ("A_far", {"initial_trust_region_radius": 1e5, "max_trust_region_radius": 1e5}),
    "13": ("A_far", {"initial_trust_region_radius": 1e5, "max_trust_region_radius": 1e5, "min_trust_region_radius": 2e3}),
    "12/1e16": ("A_far", {"initial_trust_region_radius": 1e16}),
    "13/1e16": ("A_far", {"initial_trust_region_radius": 1e16, "min_trust_region_radius": 1e14}),
    "14": (None, dict(NEGATIVE_DIAGONAL)),
    "15": (None, dict(NEGATIVE_DIAGONAL, max_consecutive_invalid_steps=1)),
    "16": (None, dict(NEGATIVE_DIAGONAL, optimize_points=0)),
    "17": ("A_nan", {}),
}
# scenarios in which nothing moves: cameras and points come back to the bit, final_cost == initial_cost
NOTHING_MOVES = ("2", "5/0", "6", "7", "8", "14", "15", "16")

# (scene, scenario) -> (termination, iterations, successful, unsuccessful) of the oracle
EXPECT = {
    ("A", "1"): (FUNCTION, 5, 4, 0),
    ("A", "2"): (GRADIENT, 0, 0, 0),
    ("A", "3A"): (GRADIENT, 3, 3, 0),
    ("A", "4"): (PARAMETER, 3, 2, 0),
    ("A", "5/0"): (NO_CONVERGENCE, 0, 0, 0),
    ("A", "5/1"): (NO_CONVERGENCE, 1, 1, 0),
    ("A", "5/3"): (NO_CONVERGENCE, 3, 3, 0),
    ("A", "6"): (TRUST_REGION, 0, 0, 0),
    ("A", "8"): (FUNCTION, 9, 0, 8),
    ("A", "11"): (FUNCTION, 14, 10, 3),
    ("A", "12"): (FUNCTION, 14, 10, 3),
    ("A", "13"): (TRUST_REGION, 6, 3, 3),
    ("A", "14"): (FAILURE, 5, 0, 4),
    ("A", "15"): (FAILURE, 1, 0, 0),
    ("A", "16"): (FAILURE, 5, 0, 4),
    ("A", "17"): (FAILURE, 0, 0, 0),
    ("C", "1"): (FUNCTION, 6, 5, 0),
    ("C", "3C"): (GRADIENT, 3, 3, 0),
    ("C", "4"): (PARAMETER, 3, 2, 0),
    ("C", "7"): (NO_CONVERGENCE, 6, 0, 6),
    ("C", "9"): (FUNCTION, 10, 1, 8),
    ("C", "10"): (TRUST_REGION, 5, 1, 4),
    ("C", "14"): (FAILURE, 5, 0, 4),
    ("C", "15"): (FAILURE, 1, 0, 0),
    ("C", "16"): (FAILURE, 5, 0, 4),
    ("E", "1"): (FUNCTION, 6, 5, 0),
    ("E", "7"): (NO_CONVERGENCE, 6, 0, 6),
    ("E", "9"): (FUNCTION, 10, 1, 8),
    ("E", "14"): (FAILURE, 5, 0, 4),
    ("E", "16"): (FAILURE, 5, 0, 4),
    ("F", "7"): (NO_CONVERGENCE, 6, 0, 6),
    ("F", "10"): (TRUST_REGION, 5, 1, 4),
}
# scenario 7: every step rejected, the radius divided by 2, 4, 8, ...
RADII_7 = (1e4, 5e3, 1250.0, 156.25, 9.765625, 0.30517578125)
# the scenarios that start far from the optimum (A_far): a rounding difference may grow along the trajectory
FAR = ("11", "12", "13")
# Scenarios 12 and 13 were first meant to start at a radius of 1e16 (the max_radius default, min_radius 1e14 for 13).
# There the first steps are Gauss-Newton steps of a system that 90 degrees from the optimum is singular to working
# precision: one ulp in the observations moves the oracle's own first step by 3 %, its third cost by 10 %, and its
# counts and even its termination with them (test_lm_cases_cpu.py).  No implementation can be held to exact counts
# there, so 12 and 13 start at 1e5 = max_trust_region_radius instead -- the cap still binds for the first three
# iterations, accepted and rejected steps still mix, 13 still ends by TRUST_REGION after rejections -- and the 1e16
# forms are kept as runs whose trajectory is not compared.
DECIDED_BY_THE_LAST_BITS = ("12/1e16", "13/1e16")


def ulp_distance(sc, opt):
    """How far apart the oracle's own results lie for two inputs that differ by one float64 ulp in every observation:
    (cameras, points) largest absolute differences, or None where the two runs did not take the same branches."""
    other = sc.copy()
    other.obs_xy = np.nextafter(sc.obs_xy, np.inf)
    s1, _, a = run_oracle(sc, opt)
    s2, _, b = run_oracle(other, opt)
    if counts(s1) != counts(s2):
        return None
    return float(np.abs(a.cam_params - b.cam_params).max()), float(np.abs(a.points - b.points).max())


def scenario_scene(base, number):
    variant, _ = SCENARIOS[number]
    if variant is None:
        return scene(base)
    assert base == "A", "the variants are of scene A"
    return scene(variant)


def scenario_options(number):
    return dict(SCENARIOS[number][1])


def run_oracle(sc, opt):
    """(summary, trace, the scene the oracle left)."""
    out = sc.copy()
    s, tr = oracle_lib.oracle_ba_solve_trace(out, **opt)
    return s, tr, out


def counts(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps)


def start_grad_max(sc, opt):
    """The gradient norm the solve tests before its first iteration."""
    o = dict(opt, gradient_tolerance=0.0, max_num_iterations=0, min_trust_region_radius=0.0)
    _, tr, _ = run_oracle(sc, o)
    return float(tr["grad_max"][0]) if tr["grad_max"].size else float("nan")     # (no rows: the cost was not finite)


def _rel(value, threshold):
    return abs(value - threshold) / abs(threshold) if threshold != 0 else np.inf


def _terms(tr, i):
    """Bound of the sum of |J step| |r| over the observations, the magnitude of the terms the model cost change is
    summed from: |r|^2 <= 2 x_cost, and |J step|^2 <= 2 model_cost_change for a Levenberg-Marquardt step
    (model_cost_change = |J step|^2 / 2 + step^T D^2 step)."""
    return 2.0 * np.sqrt(abs(tr["model_cost_change"][i]) * tr["x_cost"][i])


def margins(sc, opt, tr):
    """Every comparison the oracle made in the solve that left trace tr: a list of (iteration, name, margin)."""
    o = dict(DEFAULTS)
    o.update(opt)
    g0 = start_grad_max(sc, opt)
    if np.isnan(g0):
        return []
    out = [(0, "gradient", _rel(g0, o["gradient_tolerance"]))]
    if g0 <= o["gradient_tolerance"]:
        return out
    for i in range(tr["radius"].size):
        it = i + 1
        # FinalizeIterationAndCheckIfMinimizerCanContinue (integers: the iteration count is either there or not)
        out.append((it, "max_iterations", np.inf if i != o["max_num_iterations"] else 1.0))
        if i >= o["max_num_iterations"]:
            break
        if tr["last_successful"][i]:
            out.append((it, "gradient", _rel(tr["grad_max"][i], o["gradient_tolerance"])))
            if tr["grad_max"][i] <= o["gradient_tolerance"]:
                break
        out.append((it, "min_radius", _rel(tr["radius"][i], o["min_trust_region_radius"])))
        if tr["radius"][i] <= o["min_trust_region_radius"]:
            break
        assert tr["outcome"][i] != oracle_lib.TR_HEAD_STOP
        if tr["solve"][i] != oracle_lib.TR_SOLVED:
            out.append((it, "validity", np.inf))        # (a pivot that is not positive by many orders of magnitude)
            continue
        out.append((it, "validity", abs(tr["model_cost_change"][i]) / (1e-5 * _terms(tr, i))))
        if not tr["model_cost_change"][i] > 0:
            continue
        pt = o["parameter_tolerance"]
        out.append((it, "parameter", _rel(tr["step_norm"][i], pt * (tr["x_norm"][i] + pt))))
        if tr["outcome"][i] == oracle_lib.TR_PARAMETER_STOP:
            break
        change = tr["x_cost"][i] - tr["cand_cost"][i]
        out.append((it, "function", _rel(abs(change), o["function_tolerance"] * tr["x_cost"][i])))
        if tr["outcome"][i] == oracle_lib.TR_FUNCTION_STOP:
            break
        out.append((it, "min_relative_decrease", _rel(tr["relative_decrease"][i], o["min_relative_decrease"])))
    return out


# ---- brackets: (scene, threshold option, iteration k) ----
BRACKETS = [(s, name, k) for s in ("A", "C", "NORMS")
            for name, k in (("parameter_tolerance", 2), ("function_tolerance", 2), ("gradient_tolerance", 2),
                            ("min_relative_decrease", 2))]
NORMS_OPTIONS = {"optimize_points": 0}


def bracket_base_options(base):
    return dict(NORMS_OPTIONS) if base == "NORMS" else {}


def bracket_value(sc, base_opt, name, k):
    """What the oracle compared with the threshold `name` at iteration k of the solve with base_opt."""
    _, tr, _ = run_oracle(sc, base_opt)
    i = k - 1
    if name == "parameter_tolerance":
        # step_norm <= t (x_norm + t): the t at which it holds with equality
        t = tr["step_norm"][i] / tr["x_norm"][i]
        for _ in range(8):
            t = tr["step_norm"][i] / (tr["x_norm"][i] + t)
        return float(t)
    if name == "function_tolerance":
        return float(abs(tr["x_cost"][i] - tr["cand_cost"][i]) / tr["x_cost"][i])
    if name == "gradient_tolerance":
        # the gradient at the iterate that iteration k accepted, tested at the head of iteration k + 1
        assert tr["outcome"][i] == oracle_lib.TR_ACCEPTED and tr["last_successful"][i + 1] == 1
        return float(tr["grad_max"][i + 1])
    assert name == "min_relative_decrease"
    return float(tr["relative_decrease"][i])


def bracket_options(base_opt, name, k, value, side):
    """Options with the threshold on one side of the value: side +1 (the test holds: stop, or reject for
    min_relative_decrease) or -1.  The solve is cut short behind the decision it is about: one iteration later, or at
    once for min_relative_decrease (the step that follows a rejection has nearly the same relative decrease)."""
    o = dict(base_opt)
    o[name] = value * (1.0 + side * BRACKET)
    o["max_num_iterations"] = k if name == "min_relative_decrease" else k + 1
    return o


def bracket_expect(name, k, side):
    """What the oracle's solve must show on that side: a predicate on (counts, trace)."""
    i = k - 1
    if name == "parameter_tolerance":
        return lambda c, tr: (c[0] == PARAMETER and c[1] == k) if side > 0 else not (c[0] == PARAMETER and c[1] == k)
    if name == "function_tolerance":
        return lambda c, tr: (c[0] == FUNCTION and c[1] == k) if side > 0 else not (c[0] == FUNCTION and c[1] == k)
    if name == "gradient_tolerance":
        return lambda c, tr: (c[0] == GRADIENT and c[1] == k) if side > 0 else not (c[0] == GRADIENT and c[1] == k)
    return lambda c, tr: tr["outcome"][i] == (oracle_lib.TR_REJECTED if side > 0 else oracle_lib.TR_ACCEPTED)
