"""Mutation check of the oracle's known-answer tests (CPU only; test infrastructure).

For each mutation below -- one reference rule or quirk restated wrongly -- build a mutated copy of
oracle/apd_oracle.c into a temporary liboracle.so and run the known-answer tests against it
(APD_ORACLE_SO): the APD half's (MUTATIONS) against tests/test_oracle_kat_apd.py and
tests/test_oracle_kat.py, the Strong half's (STRONG_MUTATIONS) against
tests/test_oracle_kat_strong.py, the Weak sweep's and the moved-rig geometry's (WEAK_MUTATIONS,
GEOMETRY_MUTATIONS) against tests/test_oracle_kat_weak.py. FUSION_MUTATIONS mutate oracle/fusion_oracle.c instead and run
tests/test_oracle_kat_fusion.py plus the oracle tests of tests/test_fusion.py. A mutation the tests
do not reject ("survived") marks a rule the KATs do not pin. Usage: python tools/mutate_oracle.py
[--json apd.json] [--strong-json strong.json] [--weak-json weak.json] [--fusion-json fusion.json]
[--only apd|strong|weak|fusion]
[--jobs N]
"""
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("apd_oracle.c", "fusion_oracle.c")
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

# depth-map fusion: oracle/fusion_oracle.c (every text is one rule of the helpers, WeakVisFilter,
# RunFusion or the TAT variants; a text that occurs in several loops is mutated in all of them)
_GEO_T = ("t.x = cam->R[0] * p.x + cam->R[3] * p.y + cam->R[6] * p.z;\n"
          "    t.y = cam->R[1] * p.x + cam->R[4] * p.y + cam->R[7] * p.z;\n"
          "    t.z = cam->R[2] * p.x + cam->R[5] * p.y + cam->R[8] * p.z;")
_GEO_C = ("c.x = -(cam->R[0] * cam->t[0] + cam->R[3] * cam->t[1] + cam->R[6] * cam->t[2]);\n"
          "    c.y = -(cam->R[1] * cam->t[0] + cam->R[4] * cam->t[1] + cam->R[7] * cam->t[2]);\n"
          "    c.z = -(cam->R[2] * cam->t[0] + cam->R[5] * cam->t[1] + cam->R[8] * cam->t[2]);")
_PROJ = ("float tx = cam->R[0] * X.x + cam->R[1] * X.y + cam->R[2] * X.z + cam->t[0];\n"
         "    float ty = cam->R[3] * X.x + cam->R[4] * X.y + cam->R[5] * X.z + cam->t[1];\n"
         "    float tz = cam->R[6] * X.x + cam->R[7] * X.y + cam->R[8] * X.z + cam->t[2];")


def _transpose(text):
    for a, b in (("R[1]", "R[3]"), ("R[2]", "R[6]"), ("R[5]", "R[7]")):
        text = text.replace(a, "@").replace(b, a).replace("@", b)
    return text


_TAT_GATHER = ("f3 consistent_Point = PointX;\n                for (int j = 0; j < num_ngb; ++j) {\n"
               "                    int src_index = index_of(n, v, v[i].src_ids[j]);")
_RESET = "for (int j = 0; j < num_ngb; ++j) diff[j].dist = diff[j].depth = diff[j].angle = FLT_MAX;\n                "

FUSION_MUTATIONS = [
    ("Get3DPointonWorld: R instead of R^T on the point", "APD.cpp:875-877", _GEO_T, _transpose(_GEO_T)),
    ("Get3DPointonWorld: R instead of R^T on t", "APD.cpp:881-883", _GEO_C, _transpose(_GEO_C)),
    ("ProjectCamera: R^T instead of R", "APD.cpp:893-895", _PROJ, _transpose(_PROJ)),
    ("ProjectCamera: - t", "APD.cpp:893-895", _PROJ, _PROJ.replace("+ cam->t", "- cam->t")),
    ("Get3DPointonWorld: + R^T t", "APD.cpp:881-883", _GEO_C, _GEO_C.replace("= -(", "= (")),
    ("ProjectCamera: K[1] dropped", "APD.cpp:898",
     "cam->K[0] * tx + cam->K[1] * ty + cam->K[2] * tz", "cam->K[0] * tx + cam->K[2] * tz"),
    ("Get3DPointonWorld: y over fx", "APD.cpp:871", "(y - cam->K[5]) / cam->K[4];", "(y - cam->K[5]) / cam->K[0];"),
    ("Get3DPointonWorld: x about cy", "APD.cpp:870", "(x - cam->K[2]) / cam->K[0];", "(x - cam->K[5]) / cam->K[0];"),
    ("rounding: + 0.5f dropped", "APD.cpp:999-1000,1173-1174",
     "int_x86(py + 0.5f), src_c = int_x86(px + 0.5f)", "int_x86(py), src_c = int_x86(px)"),
    ("rounding: truncation -> floor", "APD.cpp:999-1000,1173-1174", "return (int)v;", "return (int)floorf(v);"),
    ("GetAngle: NaN -> 0 dropped", "APD.cpp:906-907", "if (angle != angle) return 0.0f;", "if (angle != angle) return 3.0f;"),
    ("RunFusion: reprojection cut 2.0 -> 1.5", "APD.cpp:1189", "reproj_error < 2.0f &&", "reproj_error < 1.5f &&"),
    ("RunFusion: relative depth cut 0.01 -> 0.008", "APD.cpp:1189",
     "relative_depth_diff < 0.01f &&", "relative_depth_diff < 0.008f &&"),
    ("RunFusion: relative depth cut 0.01 -> 0.012", "APD.cpp:1189",
     "relative_depth_diff < 0.01f &&", "relative_depth_diff < 0.012f &&"),
    ("RunFusion: angle cut 0.174533 -> 0.15", "APD.cpp:1189", "angle < 0.174533f)", "angle < 0.15f)"),
    ("RunFusion: angle cut 0.174533 -> 0.2", "APD.cpp:1189", "angle < 0.174533f)", "angle < 0.2f)"),
    ("RunFusion: 200 * rel -> 100 * rel", "APD.cpp:1192", "200 * relative_depth_diff", "100 * relative_depth_diff"),
    ("RunFusion: angle * 10 dropped", "APD.cpp:1192", " + angle * 10;", ";"),
    ("RunFusion: 0.45 / 0.3 swapped", "APD.cpp:1198", "== WEAK ? 0.45f : 0.3f", "== WEAK ? 0.3f : 0.45f"),
    ("RunFusion: colour / n instead of / (n + 1)", "APD.cpp:1215-1217", "/= (num_consistent + 1);", "/= (num_consistent);"),
    ("RunFusion: n >= 1 -> n >= 2", "APD.cpp:1199", "num_consistent >= 1 &&", "num_consistent >= 2 &&"),
    ("RunFusion: source masks not written", "APD.cpp:1209",
     "masks[src_index][(size_t)used_r[j] * v[src_index].width + used_c[j]] = 1;", ""),
    ("RunFusion: masked reference pixel not skipped", "APD.cpp:1149", "if (masks[ref_index][p] == 1) continue;", ""),
    ("masked source pixel not skipped", "APD.cpp:1176,1370,1569", "if (masks[src_index][sp] == 1) continue;", ""),
    ("RunFusion: filtered pixel not skipped", "APD.cpp:1152",
     "if (masks[ref_index][p] == 1) continue;\n                if (skip[ref_index][p] == 1) continue;",
     "if (masks[ref_index][p] == 1) continue;"),
    ("source depth <= 0 -> < 0", "APD.cpp:1179,1373,1572", "if (src_depth <= 0.0) continue;", "if (src_depth < 0.0) continue;"),
    ("NaN reference depth skipped", "APD.cpp:1157,1354,1550", "if (ref_depth <= 0.0) continue;", "if (!(ref_depth > 0.0)) continue;"),
    ("filter: STRONG reference pixels flagged too", "APD.cpp:977",
     "if (v[ref_index].weak[(size_t)r * width + c] != WEAK) continue;", "if (v[ref_index].weak[(size_t)r * width + c] == 2) continue;"),
    ("filter: view angle 80 -> 90 degrees", "APD.cpp:991", "if (angle > 80.0f) continue;", "if (angle > 90.0f) continue;"),
    ("filter: view angle in radians", "APD.cpp:990", "angle = (float)(angle * 180.0f / M_PI);", ""),
    ("filter: proj_depth <= 0 let through", "APD.cpp:997", "if (proj_depth <= 0.0f) continue;", ""),
    ("filter: occlusion margin 0.01 -> 0.02", "APD.cpp:1006,1012", "src_depth - 0.01f * src_depth", "src_depth - 0.02f * src_depth"),
    ("filter: occlusion margin dropped", "APD.cpp:1006,1012", "src_depth - 0.01f * src_depth", "src_depth"),
    ("filter: strong >= 2 -> >= 3", "APD.cpp:1019", "strong_occluded >= 2", "strong_occluded >= 3"),
    ("filter: weak >= 4 -> >= 3", "APD.cpp:1019", "weak_occluded >= 4", "weak_occluded >= 3"),
    ("filter: weak >= 4 -> >= 5", "APD.cpp:1019", "weak_occluded >= 4", "weak_occluded >= 5"),
    ("filter: confidence compare reversed", "APD.cpp:1010-1011",
     "conf_at_float(&v[src_index], src_r, src_c) < conf_at_float(&v[ref_index], r, c)",
     "conf_at_float(&v[src_index], src_r, src_c) > conf_at_float(&v[ref_index], r, c)"),
    ("filter: confidence compare <=", "APD.cpp:1010-1011",
     "conf_at_float(&v[src_index], src_r, src_c) < conf_at_float(&v[ref_index], r, c)",
     "conf_at_float(&v[src_index], src_r, src_c) <= conf_at_float(&v[ref_index], r, c)"),
    ("filter: STRONG source needs the confidence test too", "APD.cpp:1005-1008",
     "if (proj_depth < src_depth - 0.01f * src_depth) strong_occluded++;",
     "if (conf_at_float(&v[src_index], src_r, src_c) < conf_at_float(&v[ref_index], r, c) && "
     "proj_depth < src_depth - 0.01f * src_depth) strong_occluded++;"),
    ("filter: confidence read at column c, not 4c", "APD.cpp:1010-1011",
     "(size_t)r * v->width + 4 * (size_t)c;", "(size_t)r * v->width + (size_t)c;"),
    ("filter: confidence read as a byte", "APD.cpp:1010-1011",
     "float f;\n    memcpy(&f, &u, 4);\n    return f;", "return (float)b[0];"),
    ("filter: bytes past the confidence map are 0x7f", "APD.cpp:1010-1011", "v->confidence[o + k] : 0;", "v->confidence[o + k] : 0x7f;"),
    ("filter: state 2 counted as WEAK", "APD.cpp:1009", "} else if (v[src_index].weak[sp] == WEAK) {", "} else {"),
    ("TAT: cost cache reset per pixel", "APD.cpp:1347,1541", _TAT_GATHER, _RESET + _TAT_GATHER),
    ("TAT_A: colours averaged like TAT_I", "APD.cpp:1596",
     "if (variant == 1) {\n                            for (int j = 0; j < num_ngb; ++j) {", "if (1) {\n                            for (int j = 0; j < num_ngb; ++j) {"),
    ("TAT_I: reference colour alone like TAT_A", "APD.cpp:1404-1417",
     "if (variant == 1) {\n                            for (int j = 0; j < num_ngb; ++j) {", "if (0) {\n                            for (int j = 0; j < num_ngb; ++j) {"),
    ("TAT: count >= k -> count > k", "APD.cpp:1399,1593", "if (count >= k) {", "if (count > k) {"),
    ("TAT: depth_base swapped between the variants", "APD.cpp:1240,1444",
     "variant == 1 ? 1.0f / 3500.0f : 1.0f / 3000.0f", "variant == 1 ? 1.0f / 3000.0f : 1.0f / 3500.0f"),
    ("TAT: dist_base 0.25 -> 0.3", "APD.cpp:1239,1443", "const float dist_base = 0.25f;", "const float dist_base = 0.3f;"),
    ("TAT: levels start at k = 1", "APD.cpp:1389,1586", "for (int k = 2; k <= num_ngb; ++k) {", "for (int k = 1; k <= num_ngb; ++k) {"),
    ("TAT: levels stop at k = n - 1", "APD.cpp:1389,1586", "for (int k = 2; k <= num_ngb; ++k) {", "for (int k = 2; k < num_ngb; ++k) {"),
    ("TAT_A: angle cut applied as in TAT_I", "APD.cpp:1589", "if (variant == 1) pass = pass &&", "if (1) pass = pass &&"),
    ("TAT_I: angle cut dropped", "APD.cpp:1393-1394", "if (variant == 1) pass = pass &&", "if (0) pass = pass &&"),
    ("TAT_I: angle cut without angle_base", "APD.cpp:1394", "(k * angle_grad + angle_base)", "(k * angle_grad)"),
    ("TAT: masks[ref] not set", "APD.cpp:1422,1598", "masks[ref_index][p] = 1;", ""),
    ("TAT_A: skip_weak not counted", "APD.cpp:1546", "skip_weak++;", ""),
    ("TAT: levels tried from the top (the widest level wins, not the first)", "APD.cpp:1389,1586",
     "for (int k = 2; k <= num_ngb; ++k) {", "for (int k = num_ngb; k >= 2; --k) {"),
    ("index_of: a missing id reads as the last view", "APD.cpp:1143,1167", "return i;\n    return 0;", "return i;\n    return n - 1;"),
    ("index_of: last index of a repeated id", "APD.cpp:1091",
     "for (int i = 0; i < n; ++i)\n        if (v[i].ref_id == id) return i;", "for (int i = n - 1; i >= 0; --i)\n        if (v[i].ref_id == id) return i;"),
    ("RunFusion: the problem's own view instead of index_of(ref id)", "APD.cpp:1143",
     "int ref_index = index_of(n, v, v[i].ref_id);", "int ref_index = i;"),
]

# the Weak sweep: every text below is one line of k_sweep_weak (or, for rule d, of the view_selection
# it shares with the Strong sweep, or of the launch set-up), run against tests/test_oracle_kat_weak.py
_W_ADOPT = ("if (db >= o->P.depth_min && db <= o->P.depth_max && fc[mi] < cost_now) {\n"
            "            depth_now = db; pnow = newp[mi]; cost_now = fc[mi];")
_W_ARGMIN = ("{ float m = fc[0]; for (int j = 1; j < 8; ++j) if (fc[j] <= m) { m = fc[j]; mi = j; } }\n"
             "    f4 cur = RD(o, plane, c);\n    float cost_now = 0.0f;\n    for (int i = 0; i < N; ++i) {\n"
             "        float v = o_ncc_new(")
_W_INIT = ("if ((double)cost_now < (double)cost_init - 0.1) { WR(o, cost, c) = cost_now; WR(o, plane, c) = pnow; }\n"
           "        else WR(o, cost, c) = cost_init;\n    } else {\n        WR(o, cost, c) = cost_now; WR(o, plane, c) = pnow;\n"
           "    }\n    for (int i = 0; i < N; ++i) WR(o, vw, (size_t)i * o->HW + c) = vw[i];\n}\n\n/* PointinTriangle")
_W_FIT = "if (db >= o->P.depth_min && db <= o->P.depth_max && tc < cost_now) { depth_now = db; pnow = fit; cost_now = tc; }"
_W_GEOM = "flag[j] ? fmaf(gf, o_geom_cost(o, px, py, i + 1, RD(o, plane, pos[j])), v) : fmaf(gf, 3.0f, v);"

WEAK_MUTATIONS = [
    ("a: an anchor need not be STRONG to be a candidate", "APD.cu:1473",
     "if (ax == -1 || ay == -1 || RD(o, weak, ax + ay * W) != STRONG) continue;", "if (ax == -1 || ay == -1) continue;"),
    ("a: the candidate's plane is read at the WEAK pixel", "APD.cu:1481",
     "newp[i] = RD(o, plane, pos[i]);", "newp[i] = RD(o, plane, c);"),
    ("b: flagless rows hold 2.0 instead of 0", "APD.cu:1464",
     "memset(ca, 0, sizeof(ca));\n    ca[0][0] = 2.0f;\n    int flag[8] = {0}, pos[8] = {0};",
     "for (int j = 0; j < 8; ++j) for (int i = 0; i < 32; ++i) ca[j][i] = 2.0f;\n    int flag[8] = {0}, pos[8] = {0};"),
    ("b: cost_array[0][0] left at 0", "APD.cu:1464",
     "ca[0][0] = 2.0f;\n    int flag[8] = {0}, pos[8] = {0};", "ca[0][0] = 0.0f;\n    int flag[8] = {0}, pos[8] = {0};"),
    ("b: FindMinCostIndex <= -> < (Weak sweep)", "APD.cu:65,1575", _W_ARGMIN, _W_ARGMIN.replace("fc[j] <= m", "fc[j] < m")),
    ("b: flagless rows left out of the argmin", "APD.cu:1575,1594",
     _W_ARGMIN, _W_ARGMIN.replace("if (fc[j] <= m)", "if (flag[j] && fc[j] <= m)")),
    ("c: priors summed over candidates only", "APD.cu:1492",
     "if (ax == -1 || ay == -1) continue;\n        for (int j = 0; j < N; ++j) prior[j] +=",
     "if (ax == -1 || ay == -1 || RD(o, weak, ax + ay * W) != STRONG) continue;\n        for (int j = 0; j < N; ++j) prior[j] +="),
    ("c: priors 0.9 / 0.1 swapped (Weak sweep)", "APD.cu:1496-1501",
     "prior[j] += is_set(RD(o, sel, ax + ay * W), j) ? 0.9f : 0.1f;", "prior[j] += is_set(RD(o, sel, ax + ay * W), j) ? 0.1f : 0.9f;"),
    ("d: threshold 0.8 -> 0.9", "APD.cu:1506",
     "(float)(0.8 * (double)o_expf(FDIV((float)(iter * iter), (-90.0f))))",
     "(float)(0.9 * (double)o_expf(FDIV((float)(iter * iter), (-90.0f))))"),
    ("d: threshold ignores iter", "APD.cu:1506",
     "(float)(0.8 * (double)o_expf(FDIV((float)(iter * iter), (-90.0f))))", "0.8f"),
    ("d: count > 2 -> count > 3", "APD.cu:1520",
     "if (count > 2 && cf < 3) p = FDIV(tmpw, count);", "if (count > 3 && cf < 3) p = FDIV(tmpw, count);"),
    ("d: above 1.2 -> above 1.0", "APD.cu:1516", "if (c > 1.2f) cf++;", "if (c > 1.0f) cf++;"),
    ("d: fewer than 3 above 1.2 -> fewer than 4", "APD.cu:1520-1523",
     "if (count > 2 && cf < 3) p = FDIV(tmpw, count);\n        else if (cf < 3)",
     "if (count > 2 && cf < 4) p = FDIV(tmpw, count);\n        else if (cf < 4)"),
    ("d: fallback exp(-thr^2 / 0.32) -> 0.18", "APD.cu:1524",
     "p = o_expf(FDIV(thr * thr, (-0.32f)));", "p = o_expf(FDIV(thr * thr, (-0.18f)));"),
    ("d: 16 draws instead of 15", "APD.cu:1530", "for (int smp = 0; smp < 15; ++smp) {", "for (int smp = 0; smp < 16; ++smp) {"),
    ("e: no view drawn leaves cost 0, not NaN", "APD.cu:1589",
     "cost_now /= wn;\n    const float cost_init = cost_now;\n    float depth_now = depth_from_plane(cam, cur, px, py);\n"
     "    f4 pnow = cur;\n    if (flag[mi]) {\n        float db = depth_from_plane(cam, newp[mi]",
     "if (wn > 0) cost_now /= wn;\n    const float cost_init = cost_now;\n    float depth_now = depth_from_plane(cam, cur, px, py);\n"
     "    f4 pnow = cur;\n    if (flag[mi]) {\n        float db = depth_from_plane(cam, newp[mi]"),
    ("g: adoption < -> <=", "APD.cu:1596", _W_ADOPT, _W_ADOPT.replace("fc[mi] < cost_now", "fc[mi] <= cost_now")),
    ("g: adoption ignores the depth range", "APD.cu:1596", _W_ADOPT,
     _W_ADOPT.replace("db >= o->P.depth_min && db <= o->P.depth_max && ", "")),
    ("g: depth range without its ends", "APD.cu:1596", _W_ADOPT,
     _W_ADOPT.replace("db >= o->P.depth_min && db <= o->P.depth_max", "db > o->P.depth_min && db < o->P.depth_max")),
    ("g: selected_views written without adoption", "APD.cu:1600",
     "if (flag[mi]) {\n        float db = depth_from_plane(cam, newp[mi], px, py);",
     "WR(o, sel, c) = tsel;\n    if (flag[mi]) {\n        float db = depth_from_plane(cam, newp[mi], px, py);"),
    ("g: selected_views takes every view, not the weight mask", "APD.cu:1600",
     "cost_now = fc[mi];\n            WR(o, sel, c) = tsel;\n        }\n    }\n    /* PlaneHypothesisRefinementWeak",
     "cost_now = fc[mi];\n            WR(o, sel, c) = (1u << N) - 1u;\n        }\n    }\n    /* PlaneHypothesisRefinementWeak"),
    ("h: refinement not skipped for a zero fit normal", "APD.cu:1028-1030",
     "if (!(fit.x == 0 && fit.y == 0 && fit.z == 0)) {", "if (1) {"),
    ("h: the fit plane is not tried", "APD.cu:1046-1051", _W_FIT, "(void)db;"),
    ("h: the fit plane ignores the depth range", "APD.cu:1047", _W_FIT,
     _W_FIT.replace("db >= o->P.depth_min && db <= o->P.depth_max && ", "")),
    ("h: candidates built from the plane before the fit step", "APD.cu:1055-1067",
     "refine_candidates(o, px, py, &g, pnow, depth_now, dc, nc);\n#ifdef ORACLE_WEAK_STATS\n        const float thr5",
     "refine_candidates(o, px, py, &g, cur, depth_from_plane(cam, cur, px, py), dc, nc);\n#ifdef ORACLE_WEAK_STATS\n        const float thr5"),
    ("i: REFINE_INIT: cost - 0.1 -> cost (Weak sweep)", "APD.cu:1606", _W_INIT, _W_INIT.replace("cost_init - 0.1", "cost_init")),
    ("i: REFINE_INIT compares with the cost of before the launch", "APD.cu:1590,1606",
     _W_INIT, _W_INIT.replace("(double)cost_init - 0.1", "(double)RD(o, cost, c) - 0.1")),
    ("j: flagless rows add no geometric term", "APD.cu:1564", _W_GEOM, _W_GEOM.replace(": fmaf(gf, 3.0f, v);", ": v;")),
    ("j: flagless rows add geom_factor * 2", "APD.cu:1564", _W_GEOM, _W_GEOM.replace("3.0f", "2.0f")),
    ("j: candidate rows add no geometric term", "APD.cu:1561", _W_GEOM,
     "flag[j] ? v : fmaf(gf, 3.0f, v);"),
    ("j: cost_now without its geometric term (Weak sweep)", "APD.cu:1583",
     "float v = o_ncc_new(o, px, py, i + 1, cur);\n        if (geom) v = fmaf(gf, o_geom_cost(o, px, py, i + 1, cur), v);",
     "float v = o_ncc_new(o, px, py, i + 1, cur);"),
    ("k: the red Weak launch is left out", "APD.cu:1636-1652",
     "        FOR_COLOUR(o, 1, if (RD(o, weak, py * o->W + px) == WEAK) k_sweep_weak(o, px, py, it));\n    }\n}", "    }\n}"),
    ("k: launches stop at half the rows", "APD.cu:1617-1634", "int rl = 32 * ((hh + 15) / 16);", "int rl = 16 * ((hh + 15) / 16);"),
]

# geometry away from the identity, against the moved-rig tests of tests/test_oracle_kat_weak.py
_TO_WORLD = ("f4 r = {c->R[0] * p.x + c->R[3] * p.y + c->R[6] * p.z, c->R[1] * p.x + c->R[4] * p.y + c->R[7] * p.z,\n"
             "            c->R[2] * p.x + c->R[5] * p.y + c->R[8] * p.z, p.w};")
_TO_REF = ("f4 r = {c->R[0] * p.x + c->R[1] * p.y + c->R[2] * p.z, c->R[3] * p.x + c->R[4] * p.y + c->R[5] * p.z,\n"
           "            c->R[6] * p.x + c->R[7] * p.y + c->R[8] * p.z, p.w};")
_RREL = ("(double)c->R[3 * i] * r->R[3 * j] + (double)c->R[3 * i + 1] * r->R[3 * j + 1] +\n"
         "                                  (double)c->R[3 * i + 2] * r->R[3 * j + 2];")
_WP = ("float t0 = c->R[0] * X0 + c->R[3] * X1 + c->R[6] * X2;\n    float t1 = c->R[1] * X0 + c->R[4] * X1 + c->R[7] * X2;\n"
       "    float t2 = c->R[2] * X0 + c->R[5] * X1 + c->R[8] * X2;")
_PC = ("float t0 = c->R[0] * P[0] + c->R[1] * P[1] + c->R[2] * P[2] + c->t[0];\n"
       "    float t1 = c->R[3] * P[0] + c->R[4] * P[1] + c->R[5] * P[2] + c->t[1];\n"
       "    float t2 = c->R[6] * P[0] + c->R[7] * P[1] + c->R[8] * P[2] + c->t[2];")

GEOMETRY_MUTATIONS = [
    ("to_ref transposed", "APD.cu:415-423", _TO_REF, _TO_WORLD),
    ("to_world transposed", "APD.cu:405-413", _TO_WORLD, _TO_REF),
    ("R_relative with the factors swapped", "APD.cu:350-360", _RREL,
     _RREL.replace("c->R", "@").replace("r->R", "c->R").replace("@", "r->R")),
    ("reference centre from R instead of R^T", "APD.cu:362-370",
     "rC[j] = -((double)r->R[j] * r->t[0] + (double)r->R[3 + j] * r->t[1] + (double)r->R[6 + j] * r->t[2]);",
     "rC[j] = -((double)r->R[3 * j] * r->t[0] + (double)r->R[3 * j + 1] * r->t[1] + (double)r->R[3 * j + 2] * r->t[2]);"),
    ("depth_from_plane: K[0] and K[4] exchanged", "APD.cu:237-240",
     "return FDIV(-pl.w * c->K[0],\n                (((float)px - c->K[2]) * pl.x + FDIV(c->K[0], c->K[4]) * ((float)py - c->K[5]) * pl.y + c->K[0] * pl.z));",
     "return FDIV(-pl.w * c->K[4],\n                (((float)px - c->K[2]) * pl.x + FDIV(c->K[4], c->K[0]) * ((float)py - c->K[5]) * pl.y + c->K[4] * pl.z));"),
    ("precompute_homography: Kr in the place of Ks", "APD.cu:334-346",
     "double Ks[9] = {c->K[0], 0.0, c->K[2], 0.0, c->K[4], c->K[5], 0.0, 0.0, c->K[8]};",
     "double Ks[9] = {r->K[0], 0.0, r->K[2], 0.0, r->K[4], r->K[5], 0.0, 0.0, r->K[8]};"),
    ("precompute_homography: Ks in the place of Kr", "APD.cu:334-346",
     "double kr0 = r->K[0], kr2 = r->K[2], kr4 = r->K[4], kr5 = r->K[5];",
     "const apd_camera *q = &o->cam[1];\n    double kr0 = q->K[0], kr2 = q->K[2], kr4 = q->K[4], kr5 = q->K[5];"),
    ("Get3DPointonWorld_cu: R instead of R^T", "APD.cu:841-843", _WP, _transpose(_WP)),
    ("ProjectonCamera_cu: R^T instead of R", "APD.cu:856-858", _PC, _transpose(_PC)),
    ("get3d: y over fx", "APD.cu:197-202", "X[1] = FDIV(depth * (py - c->K[5]), c->K[4]);", "X[1] = FDIV(depth * (py - c->K[5]), c->K[0]);"),
]

TESTS = ["tests/test_oracle_kat_apd.py", "tests/test_oracle_kat.py"]
STRONG_TESTS = ["tests/test_oracle_kat_strong.py"]
WEAK_TESTS = ["tests/test_oracle_kat_weak.py"]
FUSION_TESTS = ["tests/test_oracle_kat_fusion.py", "tests/test_fusion.py::test_oracle_runfusion_known_answer",
                "tests/test_fusion.py::test_oracle_tat_known_answer",
                "tests/test_fusion.py::test_oracle_weak_filter_only_flags_weak"]


def run_set(mutations, tests, target="apd_oracle.c", jobs=1):
    """Mutates oracle/<target>; the other oracle source is compiled unchanged into every build."""
    src = open(os.path.join(REPO, "oracle", target)).read()
    other = [os.path.join(REPO, "oracle", f) for f in SOURCES if f != target]
    with tempfile.TemporaryDirectory() as td:
        os.symlink(os.path.join(REPO, "include"), os.path.join(td, "include"))  # the source's ../include
        env0 = dict(os.environ, APD_FUSION_KAT_CACHE=os.path.join(td, "kat_cache"))
        if target == "fusion_oracle.c":  # construct the problems once, with the unmutated oracle
            subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", tests[0], "-k",
                            "test_construction_is_guarded"], cwd=REPO, env=env0, check=True, capture_output=True)

        def one(k):
            name, ref, old, new = mutations[k]
            if src.count(old) == 0:
                return {"mutation": name, "ref": ref, "status": "NOT APPLIED (text not found)"}
            mdir = os.path.join(td, f"m{k}", "oracle")
            os.makedirs(mdir)
            os.symlink(os.path.join(REPO, "include"), os.path.join(td, f"m{k}", "include"))
            csrc = os.path.join(mdir, target)
            open(csrc, "w").write(src.replace(old, new))
            so = os.path.join(td, f"liboracle_mut{k}.so")
            subprocess.run(["gcc", *CFLAGS, "-I", os.path.join(REPO, "include"), "-shared", "-o", so, csrc, *other, "-lm"],
                           check=True, cwd=os.path.join(REPO, "oracle"))
            r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *tests],
                               cwd=REPO, env=dict(env0, APD_ORACLE_SO=so), capture_output=True, text=True)
            first = next((ln for ln in r.stdout.splitlines() if ln.startswith("FAILED")), "")
            if r.returncode != 0 and not first:  # a collection or fixture ERROR rejects nothing
                raise RuntimeError(f"pytest ended with {r.returncode} and no FAILED line:\n{r.stdout[-2000:]}")
            killed = bool(first)
            print(f"{'killed  ' if killed else 'SURVIVED'}  {name}  ({ref})  {first[7:90]}", flush=True)
            return {"mutation": name, "ref": ref, "status": "killed" if killed else "SURVIVED",
                    "by": first.replace("FAILED ", "")[:120]}

        with concurrent.futures.ThreadPoolExecutor(max(1, jobs)) as pool:
            return list(pool.map(one, range(len(mutations))))


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(8, os.cpu_count() or 1)
    bad = 0
    for half, flag, mutations, tests, target in (
            ("apd", "--json", MUTATIONS, TESTS, "apd_oracle.c"),
            ("strong", "--strong-json", STRONG_MUTATIONS, STRONG_TESTS, "apd_oracle.c"),
            ("weak", "--weak-json", WEAK_MUTATIONS + GEOMETRY_MUTATIONS, WEAK_TESTS, "apd_oracle.c"),
            ("fusion", "--fusion-json", FUSION_MUTATIONS, FUSION_TESTS, "fusion_oracle.c")):
        if only not in (None, half):
            continue
        results = run_set(mutations, tests, target, jobs)
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
