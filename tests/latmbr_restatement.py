"""Test helper: MinimumBayesRisk (lat/sausages.{h,cc}) restated line by line for ONE CompactLattice, ONE score point and one
initial hypothesis: Python floats where the reference has double, np.float32 where it has BaseFloat, math.exp / math.log1p
where it calls Exp / Log1p, one Python statement per reference statement (each cites its line of sausages.cc unless it
names another file).  OpenFst is absent, so lat/ cannot be compiled; this is the checker of csrc/kh_latmbr.hip, and
tests/test_lattice_mbr.py checks it in turn against facts that do not depend on it.

The lattice is the dict api.compact_lattice_mbr_prepare returns: CSR, top-sorted, the last state the single final state
with weight One, `state_times` per state (what PrepareLatticeAndInitStats :268-315 leaves).  The score point is applied
first, as `lattice-scale | lattice-add-penalty` in front of the program would (latbest_restatement.apply_point).

One deliberate difference: a state other than the first that no arc with a finite weight reaches has alpha = -inf, where
:125 computes exp(NaN); the library refuses such a lattice and so does this file (ValueError)."""
import math
import sys

import numpy as np

from latbest_restatement import apply_point

f32 = np.float32
K_LOG_ZERO_DOUBLE = -math.inf                                                # base/kaldi-math.h:49
K_MIN_LOG_DIFF_DOUBLE = math.log(sys.float_info.epsilon)                     # base/kaldi-math.h:45 Log(DBL_EPSILON)
DELTA = float(f32(1.0e-05))                                                  # sausages.h:132: BaseFloat, promoted where used


def log_add(x, y):
    """base/kaldi-math.h:178-195 (double)."""
    if x < y:                                                                # :180
        diff = x - y                                                         # :181
        x = y                                                                # :182
    else:
        diff = y - x                                                         # :184 (-inf - -inf = NaN, as in C)
    if diff >= K_MIN_LOG_DIFF_DOUBLE:                                        # :188 (false for NaN)
        return x + math.log1p(math.exp(diff))                                # :190
    return x                                                                 # :193


def l(a, b):
    """sausages.h:110."""
    return 0.0 if a == b else 1.0


def remove_eps(vec):
    """:75-79."""
    return [w for w in vec if w != 0]


def normalize_eps(vec):
    """:82-91."""
    out = [0]
    for w in remove_eps(vec):
        out += [w, 0]
    return out


class MinimumBayesRisk:
    """The class of sausages.h on a prepared lattice.  `trace` collects what the tests ask about and the reference does not
    keep: L_ after every AccStats, the longest run of b_arc == 3 seen, how often cases 1 and 2 of one arc hit one cell."""

    def __init__(self, L, scale, penalty, words, do_mbr=True):
        g, a, _, _ = apply_point(L, scale, penalty)
        n_states = int(L["n_states"])
        off, nxt = np.asarray(L["arc_offsets"], np.int64), np.asarray(L["arc_nextstate"], np.int64)
        self.do_mbr = bool(do_mbr)
        self.state_times = [0] + [int(t) for t in L["state_times"]]          # :283-285, 1-based
        self.N = n_states                                                    # :292
        self.pre = [[] for _ in range(n_states + 1)]                         # :293
        self.arcs = []
        for n in range(1, n_states + 1):                                     # :297
            for j in range(off[n - 1], off[n]):                              # :298
                with np.errstate(all="ignore"):
                    loglike = -(f32(g[j]) + f32(a[j]))                       # :306-307, a float sum stored to BaseFloat
                if math.isnan(float(loglike)) or float(loglike) == math.inf:
                    raise ValueError("arc %d: weight NaN or -inf" % j)
                arc = dict(word=int(L["arc_label"][j]), start_node=n, end_node=int(nxt[j]) + 1, loglike=f32(loglike))   # :303-307
                if arc["end_node"] <= n:
                    raise ValueError("arc %d: not top-sorted" % j)
                self.pre[arc["end_node"]].append(len(self.arcs))             # :311
                self.arcs.append(arc)                                        # :312
        self.R = [int(w) for w in words]                                     # :342 / :358
        self.L = 0.0                                                         # :343 / :359
        self.gamma = []
        self.times = []
        self.one_best_times = []
        self.one_best_confidences = []
        self.trace = dict(L=[], longest_run3=0, same_cell=0)
        self.iterations = 0
        self.mbr_decode()                                                    # :347 / :361

    def r(self, q):
        return self.R[q - 1]                                                 # sausages.h:113

    # ------------------------------------------------------------------ :27-69
    def mbr_decode(self):
        counter = 0
        while True:                                                          # :29
            self.R = normalize_eps(self.R)                                   # :30
            self.acc_stats()                                                 # :31
            self.iterations += 1
            delta_Q = 0.0                                                    # :32
            self.one_best_times = []                                         # :34
            self.one_best_confidences = []                                   # :35
            for q in range(len(self.R)):                                     # :39
                if self.do_mbr:                                              # :40
                    this_gamma = self.gamma[q]                               # :42
                    old_gamma, new_gamma = 0.0, float(this_gamma[0][1])      # :43
                    rq, rhat = self.R[q], this_gamma[0][0]                   # :44
                    for j in range(len(this_gamma)):                         # :45
                        if this_gamma[j][0] == rq:                           # :46
                            old_gamma = float(this_gamma[j][1])
                    delta_Q += (old_gamma - new_gamma)                       # :47
                    self.R[q] = rhat                                         # :51
                if self.R[q] != 0:                                           # :53
                    self.one_best_times.append(self.times[q])                # :54
                    confidence = f32(0.0)                                    # :55
                    for j in range(len(self.gamma[q])):                      # :56
                        if self.gamma[q][j][0] == self.R[q]:                 # :57
                            confidence = self.gamma[q][j][1]
                    self.one_best_confidences.append(confidence)             # :58
            if delta_Q == 0:                                                 # :62
                break
            if counter > 100:                                                # :63
                break                                                        # :65
            counter += 1                                                     # :29
        self.R = remove_eps(self.R)                                          # :68

    # ------------------------------------------------------------------ :93-130
    def edit_distance(self, N, Q, alpha, alpha_dash, alpha_dash_arc):
        alpha[1] = 0.0                                                       # :97
        alpha_dash[1][0] = 0.0                                               # :98
        for q in range(1, Q + 1):                                            # :99
            alpha_dash[1][q] = alpha_dash[1][q - 1] + l(0, self.r(q))        # :100
        for n in range(2, N + 1):                                            # :101
            alpha_n = K_LOG_ZERO_DOUBLE                                      # :102
            for i in self.pre[n]:                                            # :103
                arc = self.arcs[i]                                           # :104
                alpha_n = log_add(alpha_n, alpha[arc["start_node"]] + float(arc["loglike"]))   # :105
            alpha[n] = alpha_n                                               # :107
            if alpha_n == -math.inf:
                raise ValueError("state %d: alpha = -inf" % (n - 1))         # (the deliberate difference)
            for i in self.pre[n]:                                            # :109
                arc = self.arcs[i]                                           # :110
                s_a, w_a = arc["start_node"], arc["word"]                    # :111
                p_a = arc["loglike"]                                         # :112
                for q in range(Q + 1):                                       # :113
                    if q == 0:                                               # :114
                        alpha_dash_arc[q] = alpha_dash[s_a][q] + l(w_a, 0) + DELTA   # :115-116
                    else:
                        r_q = self.r(q)                                      # :118
                        a1 = alpha_dash[s_a][q - 1] + l(w_a, r_q)            # :119
                        a2 = alpha_dash[s_a][q] + l(w_a, 0) + DELTA          # :120
                        a3 = alpha_dash_arc[q - 1] + l(0, r_q)               # :121
                        alpha_dash_arc[q] = min(a1, min(a2, a3))             # :122
                    alpha_dash[n][q] += math.exp(alpha[s_a] + float(p_a) - alpha[n]) * alpha_dash_arc[q]   # :125
        return alpha_dash[N][Q]                                              # :129

    # ------------------------------------------------------------------ :133-266
    def acc_stats(self):
        N, Q = self.N, len(self.R)                                           # :136-137
        alpha = [0.0] * (N + 1)                                              # :139
        alpha_dash = [[0.0] * (Q + 1) for _ in range(N + 1)]                 # :140
        alpha_dash_arc = [0.0] * (Q + 1)                                     # :141
        beta_dash = [[0.0] * (Q + 1) for _ in range(N + 1)]                  # :142
        beta_dash_arc = [0.0] * (Q + 1)                                      # :143
        b_arc = [0] * (Q + 1)                                                # :144
        gamma = [dict() for _ in range(Q + 1)]                               # :145
        tau_b, tau_e = [0.0] * (Q + 1), [0.0] * (Q + 1)                      # :152
        st = self.state_times

        def add_to_map(i, d, m):                                             # sausages.h:136-142
            if d == 0:
                return
            if i in m:
                m[i] += d
            else:
                m[i] = d

        Ltmp = self.edit_distance(N, Q, alpha, alpha_dash, alpha_dash_arc)   # :154
        self.L = Ltmp                                                        # :159
        self.trace["L"].append(Ltmp)
        beta_dash[N][Q] = 1.0                                                # :162
        for n in range(N, 1, -1):                                            # :163
            for i in self.pre[n]:                                            # :164
                arc = self.arcs[i]                                           # :165
                s_a, w_a = arc["start_node"], arc["word"]                    # :166
                p_a = arc["loglike"]                                         # :167
                alpha_dash_arc[0] = alpha_dash[s_a][0] + l(w_a, 0) + DELTA   # :168
                for q in range(1, Q + 1):                                    # :169
                    r_q = self.r(q)                                          # :170
                    a1 = alpha_dash[s_a][q - 1] + l(w_a, r_q)                # :171
                    a2 = alpha_dash[s_a][q] + l(w_a, 0) + DELTA              # :172
                    a3 = alpha_dash_arc[q - 1] + l(0, r_q)                   # :173
                    if a1 <= a2:                                             # :174
                        if a1 <= a3:                                         # :175
                            b_arc[q] = 1; alpha_dash_arc[q] = a1
                        else:                                                # :176
                            b_arc[q] = 3; alpha_dash_arc[q] = a3
                    else:
                        if a2 <= a3:                                         # :178
                            b_arc[q] = 2; alpha_dash_arc[q] = a2
                        else:                                                # :179
                            b_arc[q] = 3; alpha_dash_arc[q] = a3
                run = 0
                for q in range(1, Q + 1):
                    run = run + 1 if b_arc[q] == 3 else 0
                    self.trace["longest_run3"] = max(self.trace["longest_run3"], run)
                    if q < Q and b_arc[q] == 2 and b_arc[q + 1] == 1:        # :188 of q + 1 and :196 of q meet in one cell
                        self.trace["same_cell"] += 1
                for q in range(Q + 1):                                       # :182
                    beta_dash_arc[q] = 0.0
                w = math.exp(alpha[s_a] + float(p_a) - alpha[n])             # the factor of :185 and :213
                for q in range(Q, 0, -1):                                    # :183
                    beta_dash_arc[q] += w * beta_dash[n][q]                  # :185
                    if b_arc[q] == 1:                                        # :187
                        beta_dash[s_a][q - 1] += beta_dash_arc[q]            # :188
                        add_to_map(w_a, beta_dash_arc[q], gamma[q])          # :190
                        tau_b[q] += st[s_a] * beta_dash_arc[q]               # :192
                        tau_e[q] += st[n] * beta_dash_arc[q]                 # :193
                    elif b_arc[q] == 2:                                      # :195
                        beta_dash[s_a][q] += beta_dash_arc[q]                # :196
                    else:                                                    # :198
                        beta_dash_arc[q - 1] += beta_dash_arc[q]             # :199
                        add_to_map(0, beta_dash_arc[q], gamma[q])            # :201
                        tau_b[q] += st[n] * beta_dash_arc[q]                 # :206
                        tau_e[q] += st[n] * beta_dash_arc[q]                 # :207
                beta_dash_arc[0] += w * beta_dash[n][0]                      # :213
                beta_dash[s_a][0] += beta_dash_arc[0]                        # :214
        for q in range(Q + 1):                                               # :217
            beta_dash_arc[q] = 0.0
        for q in range(Q, 0, -1):                                            # :218
            beta_dash_arc[q] += beta_dash[1][q]                              # :219
            beta_dash_arc[q - 1] += beta_dash_arc[q]                         # :220
            add_to_map(0, beta_dash_arc[q], gamma[q])                        # :221
            tau_b[q] += st[1] * beta_dash_arc[q]                             # :224
            tau_e[q] += st[1] * beta_dash_arc[q]                             # :225
        self.gamma_double = gamma
        self.gamma = [[] for _ in range(Q)]                                  # :237-238
        for q in range(1, Q + 1):                                            # :239
            for word in sorted(gamma[q]):                                    # :240 (std::map order)
                self.gamma[q - 1].append((word, f32(gamma[q][word])))        # :242
            # :244-245 GammaCompare sausages.h:196-206: larger posterior first, then the larger word
            self.gamma[q - 1].sort(key=lambda pr: (-float(pr[1]), -pr[0]))
        self.times = [[f32(0.0), f32(0.0)] for _ in range(Q)]                # :250-251
        for q in range(1, Q + 1):                                            # :252
            self.times[q - 1][0] = f32(tau_b[q])                             # :253
            self.times[q - 1][1] = f32(tau_e[q])                             # :254
            if q > 1 and self.times[q - 2][1] > self.times[q - 1][0]:        # :257
                avg = 0.5 * float(f32(self.times[q - 2][1] + self.times[q - 1][0]))   # :262 (a BaseFloat sum, times the double 0.5)
                self.times[q - 2][1] = self.times[q - 1][0] = f32(avg)       # :263


def mbr(L, scale, penalty, words, do_mbr=True):
    """One (lattice, point) in the layout of api.compact_lattice_mbr's per-point dict, plus the trace."""
    m = MinimumBayesRisk(L, scale, penalty, words, do_mbr)
    return dict(words=np.asarray(m.R, np.int32), bayes_risk=f32(m.L), bayes_risk_double=m.L, iterations=m.iterations,
                sausage_stats=[[(int(w), f32(p)) for w, p in b] for b in m.gamma],
                sausage_times=np.asarray([[t[0], t[1]] for t in m.times], f32).reshape(-1, 2),
                one_best_times=np.asarray([[t[0], t[1]] for t in m.one_best_times], f32).reshape(-1, 2),
                one_best_confidences=np.asarray(m.one_best_confidences, f32), trace=m.trace, gamma_double=m.gamma_double)


def best_path_words(L, scale, penalty):
    """The initial hypothesis api.compact_lattice_mbr takes without one_bests: the words of
    latbest_restatement.compact_lattice_shortest_path on the prepared lattice (final weight One at the last state)."""
    from latbest_restatement import compact_lattice_shortest_path
    n = int(L["n_states"])
    fg, fa = np.full(n, np.inf, f32), np.full(n, np.inf, f32)
    fg[n - 1] = fa[n - 1] = 0.0
    r = compact_lattice_shortest_path(dict(L, final_graph=fg, final_acoustic=fa), scale, penalty)
    if r is None:
        return None
    lab = np.asarray(L["arc_label"], np.int32)[np.asarray(r["arcs"], np.int64)] if len(r["arcs"]) else np.zeros(0, np.int32)
    return [int(w) for w in lab if w != 0]


def assert_same(got, want, what=""):
    """Every output exactly: integers, float32 bits."""
    bits = lambda x: np.asarray(x, f32).reshape(-1).view(np.int32)
    assert np.asarray(got["words"]).tolist() == np.asarray(want["words"]).tolist(), (what, "words")
    assert int(got["iterations"]) == int(want["iterations"]), (what, "iterations", got["iterations"], want["iterations"])
    assert np.array_equal(bits(got["bayes_risk"]), bits(want["bayes_risk"])), (what, "bayes_risk", got["bayes_risk"], want["bayes_risk"])
    assert len(got["sausage_stats"]) == len(want["sausage_stats"]), (what, "bins")
    for q, (gb, wb) in enumerate(zip(got["sausage_stats"], want["sausage_stats"])):
        assert [int(w) for w, _ in gb] == [int(w) for w, _ in wb], (what, "bin", q, gb, wb)
        assert np.array_equal(bits([p for _, p in gb]), bits([p for _, p in wb])), (what, "bin", q, gb, wb)
    for k in ("sausage_times", "one_best_times", "one_best_confidences"):
        assert np.asarray(got[k]).shape == np.asarray(want[k]).shape, (what, k)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, got[k], want[k])
