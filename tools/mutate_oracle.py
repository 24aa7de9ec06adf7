"""Mutation check of the oracle's known-answer tests (CPU only; test infrastructure).

For each mutation below -- one reference rule or quirk restated wrongly -- build a mutated copy of
oracle/apd_oracle.c into a temporary liboracle.so and run the known-answer tests against it
(APD_ORACLE_SO): the APD half's (MUTATIONS) against tests/test_oracle_kat_apd.py and
tests/test_oracle_kat.py, the Strong half's (STRONG_MUTATIONS) against
tests/test_oracle_kat_strong.py. A mutation the tests do not reject ("survived") marks a rule the
KATs do not pin. Usage: python tools/mutate_oracle.py [--json apd.json] [--strong-json strong.json]
[--only apd|strong]
"""
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "oracle", "apd_oracle.c")
CFLAGS = "-O2 -mfma -mavx2 -fPIC -fopenmp -ffp-contract=off -fno-fast-math -std=c11 -w".split()

MUTATIONS = [  # (name, reference lines, original text, mutated text)
    ("focal mix 0.25/0.75 -> 0.5/0.5", "APD.cu:586",
     "(float)(0.25 * (double)center_cost + 0.75 * (double)sc)", "(float)(0.5 * (double)center_cost + 0.5 * (double)sc)"),
    ("softmax weights -> plain mean", "APD.cu:431-446",
     "c[i] = o_expf(c[i] - mx); sum += c[i];", "c[i] = 1.0f; sum += c[i];"),
    ("out-of-frame anchor ignores the selected-view bit", "APD.cu:501-507",
     "if (is_set(RD(o, sel, ax + ay * W), s - 1)) { strong_costs[ns++] = COST_MAX;", "if (1) { strong_costs[ns++] = COST_MAX;"),
    ("curve peaks with >=", "APD.cu:2210",
     "if (pc[i - 1] > pc[i] && pc[i + 1] > pc[i]) {\n            is_peak[i] = 1;",
     "if (pc[i - 1] >= pc[i] && pc[i + 1] >= pc[i]) {\n            is_peak[i] = 1;"),
    ("single peak <= 0.15 -> < 0.15", "APD.cu:2226", "(pc[min_peak] <= 0.15f)", "(pc[min_peak] < 0.15f)"),
    ("peak spread / (count - 1) -> / count", "APD.cu:2243", "var /= (float)(count - 1);", "var /= (float)count;"),
    ("peak radius > -> >=", "APD.cu:2220", "abs(min_peak - 30) > weak_peak_radius", "abs(min_peak - 30) >= weak_peak_radius"),
    ("confidence starts at 0", "APD.cu:2303", "int nc = 1;", "int nc = 0;"),
    ("confidence reprojection weight 2 -> 1", "APD.cu:2305,2333",
     "if (FSQRT(dx * dx + dy * dy) <= 2.0f) nc += 2;", "if (FSQRT(dx * dx + dy * dy) <= 2.0f) nc += 1;"),
    ("confidence relative-depth 0.02 -> 0.05", "APD.cu:2336", "FDIV(fabsf(rd - refd), rd) <= 0.02f", "FDIV(fabsf(rd - refd), rd) <= 0.05f"),
    ("filter skip threshold removed", "APD.cu:1745", "if (RD(o, cost, c) < 0.001f) return;", "if (RD(o, cost, c) < 0.0f) return;"),
    ("filter even median -> upper middle", "APD.cu:1815-1816", "(n % 2 == 0) ? (f[m - 1] + f[m]) / 2 : f[m]", "f[m]"),
    ("filter y-5 tap condition y > 4 -> y > 5", "APD.cu:1755", "FADD(py > 4, upup - W * 2);", "FADD(py > 5, upup - W * 2);"),
    ("nearest: confidence filter removed", "APD.cu:2463", "if (RD(o, conf, t) < cc) continue;", ""),
    ("nearest: tie -> >=", "APD.cu:2472", "if (RD(o, conf, t) > bc) { bx = tx;", "if (RD(o, conf, t) >= bc) { bx = tx;"),
    ("anchors: >= 6 inliers -> >= 7", "APD.cu:2028", "if (tcnt < 6) continue;", "if (tcnt < 7) continue;"),
    ("anchors: > 3 directions -> > 6", "APD.cu:1965", "if (nsp <= 3) { WR(o, reliable, c) = 0; return; }", "if (nsp <= 6) { WR(o, reliable, c) = 0; return; }"),
    ("anchors: outliers kept", "APD.cu:2064-2067", "{ vx[i] = -1; vy[i] = -1; wgt[i] = FLT_MAX; continue; }", "{ wgt[i] = FLT_MAX; continue; }"),
    ("anchors: cone threshold cos(angle/2) -> cos(angle)", "APD.cu:1900,1939", "if (ca > K.thr) {", "if (ca > K.cos_a) {"),
]

# the Strong half: the PatchMatch core (every text below is one line of k_random_init, view_selection,
# refine_candidates, k_sweep_strong, o_geom_cost, k_ransac_fit or k_local_refine)
STRONG_MUTATIONS = [
    ("far line starts at 2 (up_far)", "APD.cu:1132",
     "int up_near = c - W, up_far = c - 3 * W,", "int up_near = c - W, up_far = c - 2 * W,"),
    ("10 far samples instead of 11 (left_far)", "APD.cu:1180",
     "flag[5] = 1; cmin = RD(o, cost, left_far); cminp = left_far;\n        for (int i = 1; i < 11; ++i)",
     "flag[5] = 1; cmin = RD(o, cost, left_far); cminp = left_far;\n        for (int i = 1; i < 10; ++i)"),
    ("far line step 2 -> 3 (down_far)", "APD.cu:1163",
     "int t = down_far + 2 * i * W;", "int t = down_far + 3 * i * W;"),
    ("near V of two levels (right_near)", "APD.cu:1296",
     "flag[6] = 1; cmin = RD(o, cost, right_near); cminp = right_near;\n        for (int i = 0; i < 3; ++i) {",
     "flag[6] = 1; cmin = RD(o, cost, right_near); cminp = right_near;\n        for (int i = 0; i < 2; ++i) {"),
    ("near V bound x < W - 1 - i -> x < W - 2 - i (up_near)", "APD.cu:1226",
     "if (py > 1 + i && px < W - 1 - i) { int t = up_near", "if (py > 1 + i && px < W - 2 - i) { int t = up_near"),
    ("region scan < -> <= (up_far)", "APD.cu:1145",
     "int t = up_far - 2 * i * W; if (RD(o, cost, t) < cmin)", "int t = up_far - 2 * i * W; if (RD(o, cost, t) <= cmin)"),
    ("region scan < -> <= (left_near)", "APD.cu:1273",
     "int t = left_near - (1 + i) - (i + 1) * W; if (RD(o, cost, t) < cmin)",
     "int t = left_near - (1 + i) - (i + 1) * W; if (RD(o, cost, t) <= cmin)"),
    ("FindMinCostIndex <= -> <", "APD.cu:65",
     "int mi = 0; /* FindMinCostIndex, APD.cu:60-71 */\n    { float m = fc[0]; for (int j = 1; j < 8; ++j) if (fc[j] <= m)",
     "int mi = 0; /* FindMinCostIndex, APD.cu:60-71 */\n    { float m = fc[0]; for (int j = 1; j < 8; ++j) if (fc[j] < m)"),
    ("cost_array[0][0] left at 0", "APD.cu:1120",
     "ca[0][0] = 2.0f; /* float cost_array[8][32] = {2.0f} */", "ca[0][0] = 0.0f;"),
    ("invalid rows hold 2.0 instead of 0", "APD.cu:1120",
     "memset(ca, 0, sizeof(ca));\n    ca[0][0] = 2.0f; /* float cost_array[8][32] = {2.0f} */",
     "for (int j = 0; j < 8; ++j) for (int i = 0; i < 32; ++i) ca[j][i] = 2.0f;"),
    ("view selection: above 1.2 -> above 1.0", "APD.cu:1350", "if (c > 1.2f) cf++;", "if (c > 1.0f) cf++;"),
    ("view selection: count > 2 -> count > 3", "APD.cu:1354",
     "if (count > 2 && cf < 3) p = FDIV(tmpw, count);", "if (count > 3 && cf < 3) p = FDIV(tmpw, count);"),
    ("view selection: fewer than 3 above 1.2 -> fewer than 4", "APD.cu:1354-1357",
     "if (count > 2 && cf < 3) p = FDIV(tmpw, count);\n        else if (cf < 3)",
     "if (count > 2 && cf < 4) p = FDIV(tmpw, count);\n        else if (cf < 4)"),
    ("view selection: threshold 0.8 -> 0.9", "APD.cu:1340",
     "(float)(0.8 * (double)o_expf(FDIV((float)(iter * iter), (-90.0f))))",
     "(float)(0.9 * (double)o_expf(FDIV((float)(iter * iter), (-90.0f))))"),
    ("view selection: threshold ignores iter", "APD.cu:1340",
     "(float)(0.8 * (double)o_expf(FDIV((float)(iter * iter), (-90.0f))))", "0.8f"),
    ("view selection: fallback exp(-thr^2 / 0.32) -> 0.18", "APD.cu:1358",
     "p = o_expf(FDIV(thr * thr, (-0.32f)));", "p = o_expf(FDIV(thr * thr, (-0.18f)));"),
    ("view selection priors 0.9 / 0.1 swapped (Strong sweep)", "APD.cu:1329-1334",
     "prior[j] += is_set(RD(o, sel, nb[i]), j) ? 0.9f : 0.1f;", "prior[j] += is_set(RD(o, sel, nb[i]), j) ? 0.1f : 0.9f;"),
    ("16 samples instead of 15", "APD.cu:1364", "for (int smp = 0; smp < 15; ++smp) {", "for (int smp = 0; smp < 16; ++smp) {"),
    ("REFINE_INIT: cost - 0.1 -> cost (Strong sweep)", "APD.cu:1431",
     "if ((double)cost_now < (double)cost_init - 0.1) { WR(o, cost, c) = cost_now; WR(o, plane, c) = pnow; }\n        else WR(o, cost, c) = cost_init;\n    } else {\n        WR(o, cost, c) = cost_now; WR(o, plane, c) = pnow;\n    }\n    for (int i = 0; i < N; ++i) WR(o, vw, (size_t)i * o->HW + c) = vw[i];\n}\n\n#ifdef ORACLE_WEAK_STATS",
     "if ((double)cost_now < (double)cost_init) { WR(o, cost, c) = cost_now; WR(o, plane, c) = pnow; }\n        else WR(o, cost, c) = cost_init;\n    } else {\n        WR(o, cost, c) = cost_now; WR(o, plane, c) = pnow;\n    }\n    for (int i = 0; i < N; ++i) WR(o, vw, (size_t)i * o->HW + c) = vw[i];\n}\n\n#ifdef ORACLE_WEAK_STATS"),
    ("initial views: cost <= threshold -> <", "APD.cu:765",
     "if (cv[i] <= thr) sv |= (1u << i);", "if (cv[i] < thr) sv |= (1u << i);"),
    ("initial cost: valid views are < 2.0 -> <= 2.0", "APD.cu:749", "if (v < COST_MAX) nvalid++;", "if (v <= COST_MAX) nvalid++;"),
    ("initial cost: no valid view costs 0 instead of 2.0", "APD.cu:771-773",
     "    } else {\n        WR(o, cost, c) = COST_MAX;\n    }", "    } else {\n        WR(o, cost, c) = 0.0f;\n    }"),
    ("geometric cost capped at 2 instead of 3", "APD.cu:875,901", "return fminf(3.0f, e);", "return fminf(2.0f, e);"),
    ("geometric cost: a hole costs 0 instead of 3", "APD.cu:887-889",
     "if (src_depth == 0.0f) return 3.0f;", "if (src_depth == 0.0f) return 0.0f;"),
    ("geometric cost: source depth pixel rounded instead of truncated", "APD.cu:885",
     "float src_depth = o->dep[s][trunc_clamp(sy, o->H) * o->W + trunc_clamp(sx, o->W)];\n    if (src_depth == 0.0f) return 3.0f;",
     "float src_depth = o->dep[s][trunc_clamp(sy + 0.5f, o->H) * o->W + trunc_clamp(sx + 0.5f, o->W)];\n    if (src_depth == 0.0f) return 3.0f;"),
    ("sweep ignores use_impetus's geometric term", "APD.cu:1406-1408",
     "const int geom_imp = o->P.geom_consistency && o->P.use_impetus;", "const int geom_imp = 0;"),
    ("refinement: depth perturbation 2 % -> 5 %", "APD.cu:961,971-972",
     "const float dminp = (1 - 0.02f) * dp;\n    const float dmaxp = (1 + 0.02f) * dp;",
     "const float dminp = (1 - 0.05f) * dp;\n    const float dmaxp = (1 + 0.05f) * dp;"),
    ("refinement: normal perturbation 0.02 pi -> 0.05 pi", "APD.cu:962,976",
     "const float pert = (float)((double)0.02f * M_PI_D);", "const float pert = (float)((double)0.05f * M_PI_D);"),
    ("refinement: candidate 3 takes the random normal", "APD.cu:980",
     "ncand[0] = cur; ncand[1] = nrand; ncand[2] = nrand; ncand[3] = npert; ncand[4] = cur;",
     "ncand[0] = cur; ncand[1] = nrand; ncand[2] = nrand; ncand[3] = nrand; ncand[4] = cur;"),
    ("refinement: random normal not turned to the camera", "APD.cu:261-265",
     "if (dot > 0.0f) { n.x = -n.x; n.y = -n.y; n.z = -n.z; }\n    normalize3(&n);", "normalize3(&n);"),
    ("RANSAC fit: fewer than 3 anchors -> fewer than 4", "APD.cu:2525",
     "if (cnt < 3) { WR(o, fit, c) = RD(o, plane, c); return; }", "if (cnt < 4) { WR(o, fit, c) = RD(o, plane, c); return; }"),
    ("RANSAC fit: plane not turned to the camera", "APD.cu:2586-2591",
     "if (dot > 0) { best.x = -best.x; best.y = -best.y; best.z = -best.z; best.w = -best.w; }", ""),
    ("RANSAC fit: no triangle leaves the pixel's plane", "APD.cu:2595-2596",
     "f4 z = {0, 0, 0, 0};\n        WR(o, fit, c) = z;", "WR(o, fit, c) = RD(o, plane, c);"),
    ("LocalRefine: radius 5 -> 4", "APD.cu:2402", "for (int pd = -5; pd <= 5; ++pd) {", "for (int pd = -4; pd <= 4; ++pd) {"),
    ("LocalRefine: better by 0.1 -> by 0", "APD.cu:2429",
     "if ((double)(cost_now - min_cost) > 0.1) WR(o, plane, c).w = best;", "if ((double)(cost_now - min_cost) > 0.0) WR(o, plane, c).w = best;"),
]

TESTS = ["tests/test_oracle_kat_apd.py", "tests/test_oracle_kat.py"]
STRONG_TESTS = ["tests/test_oracle_kat_strong.py"]


def run_set(mutations, tests):
    src = open(SRC).read()
    results = []
    with tempfile.TemporaryDirectory() as td:
        os.symlink(os.path.join(REPO, "include"), os.path.join(td, "include"))  # the source's ../include
        for name, ref, old, new in mutations:
            n = src.count(old)
            if n == 0:
                results.append({"mutation": name, "ref": ref, "status": "NOT APPLIED (text not found)"})
                continue
            mdir = os.path.join(td, "oracle")
            os.makedirs(mdir, exist_ok=True)
            csrc = os.path.join(mdir, "apd_oracle.c")
            open(csrc, "w").write(src.replace(old, new))
            so = os.path.join(td, "liboracle_mut.so")
            inc = os.path.join(REPO, "include")
            subprocess.run(["gcc", *CFLAGS, "-I", inc, "-shared", "-o", so, csrc,
                            os.path.join(REPO, "oracle", "fusion_oracle.c"), "-lm"], check=True,
                           cwd=os.path.join(REPO, "oracle"))
            env = dict(os.environ, APD_ORACLE_SO=so)
            r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *tests],
                               cwd=REPO, env=env, capture_output=True, text=True)
            killed = r.returncode != 0
            first = next((ln for ln in r.stdout.splitlines() if ln.startswith("FAILED")), "")
            results.append({"mutation": name, "ref": ref, "status": "killed" if killed else "SURVIVED",
                            "by": first.replace("FAILED ", "")[:120]})
            print(f"{'killed  ' if killed else 'SURVIVED'}  {name}  ({ref})  {first[7:90]}", flush=True)
    return results


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    bad = 0
    for half, flag, mutations, tests in (("apd", "--json", MUTATIONS, TESTS),
                                         ("strong", "--strong-json", STRONG_MUTATIONS, STRONG_TESTS)):
        if only not in (None, half):
            continue
        results = run_set(mutations, tests)
        if flag in sys.argv:
            with open(sys.argv[sys.argv.index(flag) + 1], "w") as fh:
                json.dump(results, fh, indent=1)
                fh.write("\n")
        survived = [r for r in results if r["status"] != "killed"]
        print(f"{half} half: {len(results) - len(survived)}/{len(results)} mutations killed", flush=True)
        bad += len(survived)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
