"""A line-by-line restatement of acc-tree-stats and sum-tree-stats (test infrastructure; nothing here calls the product):

  Tables                 TransitionModel::ComputeDerived and the accessors the code below uses (hmm/transition-model.cc)
  is_reordered, split_to_phones_internal, split_to_phones     hmm/hmm-utils.cc:594-701
  map_phone, accumulate_tree_stats, read_phone_map            hmm/tree-accu.cc
  GaussClusterable       AddStats / Add / Write (tree/clusterable-classes.cc:137-178): count_ a double, stats_ two rows of
                         doubles; row 0 adds double(x[d]); row 1 adds double(fl32(x[d] * x[d])) - AddVec2's alpha == 1.0
                         branch (matrix/kaldi-vector.cc:1044-1049) multiplies two floats
  acc_tree_stats         the main loop of bin/acc-tree-stats.cc:106-156
  write_tree_stats       WriteBuildTreeStats / WriteEventType (tree/build-tree-utils.cc:29-43, tree/event-map.cc:228-237)
  sum_tree_stats         the merge and the exit status of bin/sum-tree-stats.cc:54-90
  add_stats              AddStats over (frame, event) pairs in frame order: what kh_tree_acc_stats is held to, bit for bit

The sums are numpy float32 products and float64 adds made one frame after another: the order and the roundings of the
reference's loops."""
import struct

import numpy as np

K_PDF_CLASS = -1          # kPdfClass (tree/context-dep.h)
K_NO_PDF = -1             # kNoPdf (hmm/hmm-topology.h)


class KaldiAssert(Exception):
    pass


class KaldiErr(Exception):
    pass


class Tables:
    """topo: dict(phones, phone2idx, entries[i][j] = (pdf_class, [(dst, prob), ...])); triples: [(phone, hmm_state, pdf)]."""

    def __init__(self, topo, triples):
        self.topo, self.triples = topo, [tuple(int(x) for x in t) for t in triples]
        self.state2id, self.id2state = [0], [0]               # ComputeDerived :72-98
        cur = 1
        for tstate in range(1, len(self.triples) + 1):
            self.state2id.append(cur)
            phone, hmm_state, _ = self.triples[tstate - 1]
            for _ in self.entry(phone)[hmm_state][1]:
                self.id2state.append(tstate)
                cur += 1
        self.state2id.append(cur)

    def entry(self, phone):
        return self.topo["entries"][self.topo["phone2idx"][phone]]

    def num_transition_ids(self):
        return len(self.id2state) - 1

    def tid_to_tstate(self, tid):
        return self.id2state[tid]

    def tid_to_tindex(self, tid):
        return tid - self.state2id[self.id2state[tid]]

    def tstate_to_phone(self, tstate):
        return self.triples[tstate - 1][0]

    def tstate_to_hmm_state(self, tstate):
        return self.triples[tstate - 1][1]

    def tid_to_phone(self, tid):
        return self.tstate_to_phone(self.id2state[tid])

    def tid_to_pdf_class(self, tid):                          # TransitionIdToPdfClass
        phone, hmm_state, _ = self.triples[self.id2state[tid] - 1]
        return self.entry(phone)[hmm_state][0]

    def is_self_loop(self, tid):                              # :217-225
        _, hmm_state, _ = self.triples[self.id2state[tid] - 1]
        phone = self.tid_to_phone(tid)
        return self.entry(phone)[hmm_state][1][self.tid_to_tindex(tid)][0] == hmm_state

    def is_final(self, tid):                                  # :200-215
        phone, hmm_state, _ = self.triples[self.id2state[tid] - 1]
        entry = self.entry(phone)
        return entry[hmm_state][1][self.tid_to_tindex(tid)][0] + 1 == len(entry)


def is_reordered(tm, alignment):
    for i in range(len(alignment) - 1):
        tstate1, tstate2 = tm.tid_to_tstate(alignment[i]), tm.tid_to_tstate(alignment[i + 1])
        if tstate1 != tstate2:
            is_loop_1, is_loop_2 = tm.is_self_loop(alignment[i]), tm.is_self_loop(alignment[i + 1])
            if is_loop_1 and is_loop_2:
                raise KaldiAssert("!(is_loop_1 && is_loop_2)")
            if is_loop_1:
                return True
            if is_loop_2:
                return False
    if len(alignment) == 0:
        return False
    if tm.is_self_loop(alignment[0]):
        return False
    if tm.is_self_loop(alignment[-1]):
        return True
    return False


def split_to_phones_internal(tm, alignment, reordered, split_output):
    if len(alignment) == 0:
        return True
    end_points = []
    was_ok = True
    i = 0
    while i < len(alignment):
        trans_id = alignment[i]
        if tm.is_final(trans_id):
            if not reordered:
                end_points.append(i + 1)
            else:
                while i + 1 < len(alignment) and tm.is_self_loop(alignment[i + 1]):
                    if tm.tid_to_tstate(alignment[i]) != tm.tid_to_tstate(alignment[i + 1]):
                        raise KaldiAssert("TransitionIdToTransitionState(alignment[i]) == TransitionIdToTransitionState(alignment[i+1])")
                    i += 1
                end_points.append(i + 1)
        elif i + 1 == len(alignment):
            was_ok = False
            end_points.append(i + 1)
        else:
            this_state, next_state = tm.tid_to_tstate(alignment[i]), tm.tid_to_tstate(alignment[i + 1])
            if this_state != next_state:
                this_phone, next_phone = tm.tstate_to_phone(this_state), tm.tstate_to_phone(next_state)
                if this_phone != next_phone:
                    was_ok = False
                    end_points.append(i + 1)
        i += 1
    cur_point = 0
    for end in end_points:
        split_output.append([])
        trans_state = tm.tid_to_tstate(alignment[cur_point])
        phone = tm.tstate_to_phone(trans_state)
        pdf_class = tm.entry(phone)[0][0]
        if pdf_class != K_NO_PDF:
            if tm.tstate_to_hmm_state(trans_state) != 0:
                was_ok = False
        for j in range(cur_point, end):
            split_output[-1].append(alignment[j])
        cur_point = end
    return was_ok


def split_to_phones(tm, alignment, split_alignment):
    del split_alignment[:]
    return split_to_phones_internal(tm, alignment, is_reordered(tm, alignment), split_alignment)


def map_phone(phone_map, phone):
    if phone == 0 or phone_map is None:
        return phone
    if phone < 0 or phone >= len(phone_map):
        raise KaldiErr("Out-of-range phone %d bad --phone-map option?" % phone)
    return int(phone_map[phone])


class GaussClusterable:
    def __init__(self, dim, var_floor):
        self.count = np.float64(0.0)
        self.var_floor = float(np.float32(var_floor))         # a double that holds the float option
        self.stats = np.zeros((2, dim), np.float64)

    def add_stats(self, vec, weight=np.float32(1.0), double_products=False):
        vec = np.asarray(vec, np.float32)
        assert weight == 1.0                                   # the alpha == 1.0 branches are the ones restated
        self.count = self.count + np.float64(weight)
        self.stats[0] += vec.astype(np.float64)                # data_[i] += other[i]
        if double_products:                                    # NOT the reference: the cases' sensitivity check
            self.stats[1] += vec.astype(np.float64) * vec.astype(np.float64)
        else:
            self.stats[1] += (vec * vec).astype(np.float64)    # data_[i] += other[i] * other[i], float operands

    def add(self, other):
        self.count = self.count + other.count
        self.stats += other.stats                              # AddMat(1.0)

    def as_dict(self):
        return dict(count=float(self.count), var_floor=self.var_floor, stats=self.stats)


def window_events(tm, N, P, ci_phones, split_alignment, phone_map):
    """The loops of AccumulateTreeStats :56-104 without the statistics: yields (cur_pos, evec_more) frame after frame, then
    checks cur_pos against the alignment's length."""
    cur_pos = 0
    n_split = len(split_alignment)
    for i in range(-N, n_split):
        if i + P >= 0 and i + P < n_split:
            central_phone = map_phone(phone_map, tm.tid_to_phone(split_alignment[i + P][0]))
            is_ctx_dep = central_phone not in ci_phones
            evec = []
            for j in range(N):
                if i + j >= 0 and i + j < n_split:
                    phone = map_phone(phone_map, tm.tid_to_phone(split_alignment[i + j][0]))
                else:
                    phone = 0
                if is_ctx_dep or j == P:
                    evec.append((j, phone))
            for j in range(len(split_alignment[i + P])):
                evec_more = list(evec)
                evec_more.append((K_PDF_CLASS, tm.tid_to_pdf_class(split_alignment[i + P][j])))
                evec_more.sort()
                yield cur_pos, tuple(evec_more)
                cur_pos += 1
    if cur_pos != sum(len(s) for s in split_alignment):
        raise KaldiAssert("cur_pos == static_cast<int>(alignment.size())")


def accumulate_tree_stats(tm, var_floor, N, P, ci_phones, alignment, features, phone_map, stats, events_out=None):
    """AccumulateTreeStats; stats: dict event -> GaussClusterable.  False: "alignment appears to be bad, not using it"."""
    ci_phones = list(ci_phones)
    if any(a >= b for a, b in zip(ci_phones, ci_phones[1:])):
        raise KaldiAssert("IsSortedAndUniq(ci_phones)")
    split_alignment = []
    if not split_to_phones(tm, list(alignment), split_alignment):
        return False
    assert features is None or features.shape[0] == len(alignment)
    for cur_pos, event in window_events(tm, N, P, ci_phones, split_alignment, phone_map):
        if events_out is not None:
            events_out.append(event)
        if features is not None:
            if event not in stats:
                stats[event] = GaussClusterable(features.shape[1], var_floor)
            stats[event].add_stats(features[cur_pos])
    return True


def frame_events(tm, alignment, N, P, ci_phones, phone_map):
    """(ok, the events frame by frame) of one alignment."""
    events = []
    ok = accumulate_tree_stats(tm, 0.01, N, P, ci_phones, alignment, None, phone_map, None, events_out=events)
    return ok, events if ok else []


def read_phone_map(text):
    phone_map = []
    lines = text.split("\n")
    if lines[-1] == "":
        lines.pop()
    for i, line in enumerate(lines):
        try:
            v = [int(w) for w in line.replace("\t", " ").replace("\r", " ").split(" ") if w]
        except ValueError:
            raise KaldiErr("Error reading phone map")
        if len(v) != 2 or v[0] <= 0 or v[1] <= 0 or (v[0] < len(phone_map) and phone_map[v[0]] != -1):
            raise KaldiErr("(bad line %d)" % i)
        if v[0] >= len(phone_map):
            phone_map += [-1] * (v[0] + 1 - len(phone_map))
        phone_map[v[0]] = v[1]
    if not phone_map:
        raise KaldiErr("Read empty phone map")
    return phone_map


def acc_tree_stats(tm, job, var_floor=0.01, N=3, P=1, ci_phones=(), phone_map=None):
    """job: [(features or None-for-no-alignment ..)] as [(mat, alignment or None)] in the feature archive's order ->
    (stats in std::map order as [(event, dict)], num_done, num_no_alignment, num_other_error, bad alignments)."""
    tree_stats = {}
    num_done = num_no_alignment = num_other_error = num_bad = 0
    for mat, alignment in job:
        if alignment is None:
            num_no_alignment += 1
            continue
        if len(alignment) != mat.shape[0]:
            num_other_error += 1
            continue
        if not accumulate_tree_stats(tm, var_floor, N, P, ci_phones, alignment, mat, phone_map, tree_stats):
            num_bad += 1
        num_done += 1
    stats = [(event, tree_stats[event].as_dict()) for event in sorted(tree_stats)]     # std::map<EventType>: pairs in turn
    return stats, num_done, num_no_alignment, num_other_error, num_bad


def _g7(x):
    x = float(x)                                               # operator<< at 7 significant digits
    return "%.7g" % x


def write_tree_stats(stats, binary):
    """The bytes WriteBuildTreeStats writes after Output's header; stats: [(event, dict or None)]."""
    out = []
    if binary:
        out.append(b"BTS " + b"\xfc" + struct.pack("<I", len(stats)))
        for event, gc in stats:
            out.append(b"EV " + b"\xfc" + struct.pack("<I", len(event)))
            for k, v in event:
                out.append(b"\x04" + struct.pack("<i", k) + b"\x04" + struct.pack("<i", v))
            out.append(b"T" if gc is not None else b"F")
            if gc is not None:
                m = np.ascontiguousarray(gc["stats"], "<f8")
                out.append(b"GCL " + b"\x08" + struct.pack("<d", gc["count"]) + b"\x08" + struct.pack("<d", gc["var_floor"]))
                out.append(b"DM " + b"\x04" + struct.pack("<i", m.shape[0]) + b"\x04" + struct.pack("<i", m.shape[1]) + m.tobytes())
    else:
        out.append(b"BTS %d " % len(stats))
        for event, gc in stats:
            out.append(b"EV %d " % len(event) + b"".join(b"%d %d " % (k, v) for k, v in event) + b"\n")
            out.append(b"T " if gc is not None else b"F ")
            if gc is not None:
                out.append(("GCL %s %s " % (_g7(gc["count"]), _g7(gc["var_floor"]))).encode())
                m = np.asarray(gc["stats"], np.float64)
                if m.size == 0:
                    out.append(b" [ ]\n")
                else:
                    out.append(b" [" + b"".join(b"\n  " + b"".join((_g7(x) + " ").encode() for x in row) for row in m) + b"]\n")
        out.append(b"\n")
    return b"".join(out)


def sum_tree_stats(files):
    """files: [[(event, dict)]] in argument order -> (the summed stats in std::map order, exit status)."""
    tree_stats = {}
    for stats_array in files:
        for event, c in stats_array:
            g = GaussClusterable(c["stats"].shape[1], 0.0)
            g.count, g.var_floor, g.stats = np.float64(c["count"]), c["var_floor"], np.array(c["stats"], np.float64)
            if event not in tree_stats:
                tree_stats[event] = g
            else:
                tree_stats[event].add(g)
    stats = [(event, tree_stats[event].as_dict()) for event in sorted(tree_stats)]
    return stats, 0 if len(stats) != 0 else 1


def add_stats(feats, frame_event, num_events, count=None, stats=None, double_products=False):
    """GaussClusterable::AddStats for the frames t = 0, 1, ... with frame_event[t] >= 0, on from (count, stats) or from zero
    -> (count [E], stats [E, 2, D]) float64."""
    feats = np.asarray(feats, np.float32)
    D = feats.shape[1]
    gcs = [GaussClusterable(D, 0.01) for _ in range(num_events)]
    for e in range(num_events):
        if count is not None:
            gcs[e].count = np.float64(count[e])
            gcs[e].stats = np.array(stats[e], np.float64)
    for t, e in enumerate(np.asarray(frame_event).tolist()):
        if e >= 0:
            gcs[e].add_stats(feats[t], double_products=double_products)
    return (np.array([g.count for g in gcs], np.float64).reshape(num_events),
            np.array([g.stats for g in gcs], np.float64).reshape(num_events, 2, D))
