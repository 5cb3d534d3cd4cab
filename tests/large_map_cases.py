"""Case tables of test_large_map_hooks_cpu.py and test_large_map_kernels_gpu.py: maps beyond 66 landmarks, up to the capacity of 1000, for
the kernels around the step.  Every edge is derived from the source it names; the launch rules are restated here in a few lines and the
tables are asserted against them on the CPU (test_premises_* of the CPU module).  A helper: no tests in here."""
import math

import numpy as np

import fix_reference as FR
import map_reference as MR
import merge_reference as R

CAPACITY = 1000                        # kMapMaxLandmarks (map_kernel.h): the largest L_max a handle accepts
E1, E2 = (0.8, 0.3), (-0.5, 0.9)       # displacements of a copy in units of its noise: d2 = 0.365 and 0.53 (test_merge_reference.py)


def ekf_ld(n, esz):
    """ekf_ld (ekf_kernel.h): the leading dimension of P, 16-byte rows."""
    return (n + 1) & ~1 if esz == 8 else (n + 3) & ~3


# ---- launch_merge_find / launch_merge_fuse (merge_kernel.hip) restated ---------------------------------------------------------------------
def merge_find_rule(L_max):
    """kind 0: L_max <= 64, four wavefronts share the slots t; kind 1: <= 256, one slot per lane; kind 2: up to kMergeOwn = 4 slots per
    lane, j = tid + k * 256.  The panel depth TP is what kMergePanelBytes = 56 KiB hold of 32 npad bytes per slot, 1 .. 8; the launch
    raises the kernel's LDS limit where the panels and 8 KiB of static LDS exceed 64 KiB."""
    npad = (3 + 2 * L_max) | 1
    TP = min(max(57344 // (32 * npad), 1), 8)
    lds = 8 * 4 * TP * npad
    return dict(kind=0 if L_max <= 64 else (1 if L_max <= 256 else 2), TP=TP, npad=npad, lds=lds, full_lds=lds + 8192 > 64 * 1024)


def merge_fuse_rule(L_max):
    """The workspace of 4 n + 2 doubles at n = 3 + 2 L_max; the limit is raised where it and 4 KiB of static LDS exceed 64 KiB."""
    lds = 8 * (4 * (3 + 2 * L_max) + 2)
    return dict(lds=lds, full_lds=lds + 4096 > 64 * 1024)


def owned_round(slot):
    """k of j = tid + k * 256: which of a lane's (up to four) slots `slot` is."""
    return slot // 256


def compact_chunks(M_after, esz):
    """map_compact_kernel gathers the n' * ld' elements of the compacted P in chunks of 256 lanes x kMapChunk = 8 elements."""
    n2 = 3 + 2 * M_after
    return -(-(n2 * ekf_ld(n2, esz)) // 2048)


# ---- 4. duplicate find and merge ----------------------------------------------------------------------------------------------------------
# L_max -> (kind, TP, find raises the LDS limit, fuse raises it) as the issue's table states them; asserted against the rules above
MERGE_TABLE = {64: (0, 8, False, False), 65: (1, 8, False, False), 126: (1, 7, False, False), 147: (1, 6, False, False),
               177: (1, 5, False, False), 222: (1, 4, False, False), 256: (1, 3, False, False), 257: (2, 3, False, False),
               297: (2, 3, False, False), 447: (2, 1, False, False), 512: (2, 1, False, False), 513: (2, 1, False, False),
               768: (2, 1, False, False), 769: (2, 1, False, False), 894: (2, 1, False, False), 895: (2, 1, True, False),
               958: (2, 1, True, False), 959: (2, 1, True, True), 1000: (2, 1, True, True)}
# both storage types up to 513 (every kind, every TP, the third owned slot); one each beyond, alternating, so that both instantiations of
# the find and of the fuse launch above 64 KiB
MERGE_CASES = [(L, f32) for L in sorted(MERGE_TABLE) if L <= 513 for f32 in (False, True)] + \
              [(768, False), (769, True), (894, True), (895, False), (958, False), (959, True), (1000, False), (1000, True)]
MERGE_IDS = [f"L{L}_{'f32' if f32 else 'f64'}" for L, f32 in MERGE_CASES]
PAIRS = ((5, 261), (255, 256), (300, 700), (511, 512), (767, 768), (2, -1), (40, 41), (63, 64), (17, 50))
CHAINS = ((10, 270, 530), (10, 75, 140), (10, 30, 60))


def merge_counts(L_max):
    """The landmark counts of a handle's three instances: full, one and two below capacity (so at least two of them are no multiple of
    any TP >= 3, and the handle of 1000 holds 998 - 1000)."""
    return (L_max, L_max - 1, L_max - 2)


def merge_layout(M):
    """(copies of merge_reference.layout_with, the mutual pairs, the chain (a, b, c) whose c is not mutual): the placements of PAIRS that
    fit into M slots ((2, -1) is (2, M - 1)), and the first chain of CHAINS that fits.  A chain a - b - c holds copies of one landmark
    with d2(a, b) = 0.125, d2(a, c) = 1.125 and d2(b, c) = 2, as test_merge_reference's: c's best candidate is a, a's is b."""
    used, copies, pairs = set(), {}, []
    chain = next(c for c in CHAINS if c[2] < M)
    copies[chain[1]] = (chain[0], (0.5, 0.0), True); copies[chain[2]] = (chain[0], (-1.5, 0.0), True)
    used.update(chain)
    for k, (i, j) in enumerate(PAIRS):
        j = M + j if j < 0 else j
        if j < M and i not in used and j not in used:
            copies[j] = (i, E1 if k % 2 else E2, True)
            pairs.append((i, j)); used.update((i, j))
    return copies, pairs, chain


def merge_by_pairs(L_max, f32):
    """The fp64 handles up to 513 fuse through slam_merge_landmarks with the pairs the find returned (and two entries to ignore); the
    others through slam_map_merge."""
    return not f32 and L_max <= 513


def caller_pairs(found, chain, M, L_max):
    """The find's partner row with an entry that is not mutual (the chain's c names a) and, where the map has room, one at a slot that
    holds no landmark: (row, entries to ignore)."""
    row = np.array(found, dtype=np.int32)
    row[chain[2]] = chain[0]
    if M < L_max:
        row[L_max - 1] = 1000000
    return row, 1 + int(M < L_max)


def merge_state(L_max, M, f32, seed=0):
    rng = np.random.default_rng(1000 * L_max + M + 7 * int(f32) + seed)
    copies, pairs, chain = merge_layout(M)
    st = R.crafted_state(rng, R.layout_with(M, copies), f32)
    return st, pairs, chain


# ---- 3. map removal, tally and prune -------------------------------------------------------------------------------------------------------
MAP_COUNTS = (64, 65, 128, 129, 1000)
NEW_REMOVAL_SETS = ("exactly slots 63 and 64", "one whole 64-slot trip", "every slot but the last")
REMOVAL_SETS = MR.REMOVAL_SETS + ("random",) + NEW_REMOVAL_SETS
TALLY_LENGTHS = (63, 64, 65, 128, 129)                  # kMapIdBlock = 64 (map_kernel.h): one block less one, one, one and one id, two, two and one
# (L_max, landmarks, fp32 storage): every count full and one below capacity once; both storage types up to 129, fp32 at the capacity
MAP_CASES = [(64, 64, False), (65, 64, True), (65, 65, False), (66, 65, True), (128, 128, True), (129, 128, False), (129, 129, True),
             (130, 129, False), (1000, 1000, True), (1000, 999, True)]
MAP_IDS = [f"L{L}_M{M}_{'f32' if f32 else 'f64'}" for L, M, f32 in MAP_CASES]


def removal_mask(kind, M, rng=None):
    """map_reference.removal_mask and the three sets that sit on the 64-slot trips in which wavefront 0 builds the kept list
    (map_kernel.hip: ballot positions in a uint16 table)."""
    m = np.zeros(M, dtype=np.int32)
    if kind == "exactly slots 63 and 64":
        m[63:65] = 1                                     # (at M = 64 slot 63 alone: the last lane of the only trip)
    elif kind == "one whole 64-slot trip":
        lo = 64 if M >= 128 else 0
        m[lo:lo + 64] = 1
    elif kind == "every slot but the last":
        m[:M - 1] = 1
    else:
        return MR.removal_mask(kind, M, rng)
    return m


# (case) -> the chunks of 2048 elements the compaction of P takes per removal set, in the order of FIXED_REMOVAL_SETS (0: nothing moves):
# n' ld' / 2048 rounded up at n' = 3 + 2 M', ld' = ekf_ld(n') (e.g. 1000 landmarks less slots 63 and 64 in fp32: 1999 x 2000 / 2048 =
# 1952.1); literal expectations, asserted on the CPU for every case and set
FIXED_REMOVAL_SETS = tuple(k for k in REMOVAL_SETS if k != "random")
MAP_CHUNKS = {(64, 64, False): (0, 9, 9, 1, 3, 1, 9, 1, 1),
              (65, 64, True): (0, 9, 9, 1, 3, 1, 9, 1, 1),
              (65, 65, False): (0, 9, 9, 1, 3, 1, 9, 1, 1),
              (66, 65, True): (0, 9, 9, 1, 3, 1, 9, 1, 1),
              (128, 128, True): (0, 33, 33, 1, 9, 1, 32, 9, 1),
              (129, 128, False): (0, 33, 33, 1, 9, 1, 32, 9, 1),
              (129, 129, True): (0, 33, 33, 1, 9, 1, 33, 9, 1),
              (130, 129, False): (0, 33, 33, 1, 9, 1, 33, 9, 1),
              (1000, 1000, True): (0, 1959, 1959, 1, 492, 1, 1953, 1718, 1),
              (1000, 999, True): (0, 1953, 1953, 1, 491, 1, 1951, 1716, 1)}


def tally_message(rng, st, k):
    """k ids: every third one an id that is not in the map or no id at all, the others mapped slots taken from every 64-slot trip."""
    m = MR.crafted_message(rng, st, k, hits=0.0)
    M = st["M"]
    trips, q = -(-M // 64), 0
    for l in range(k):
        if l % 3:
            m[l, 0] = float(st["ids"][min((q % trips) * 64 + (5 * (q // trips)) % 64, M - 1)])
            q += 1
    m[k - 1, 0] = float(st["ids"][M - 1])               # the last id of the message names the last slot
    return m


# ---- 5. fixes ----------------------------------------------------------------------------------------------------------------------------------
# fix_instance_kernel (fix_kernel.hip): 256 lanes over the n = 3 + 2 M rows, n in {255, 257, 511, 513, 2003}: one below and one above a
# whole number of passes of the lanes, and the capacity.  launch_fix raises the kernel's LDS limit where the workspace of fix_ws_len(n) =
# 6 n + 3 doubles at n = 3 + 2 L_max and 4 KiB of static LDS exceed 64 KiB: from L_max 639, run on both sides and in both storage types.
FIX_COUNTS = (126, 127, 254, 255, 1000)
FIX_CASES = [(126, 126, False), (127, 126, True), (127, 127, False), (128, 127, True), (254, 254, True), (255, 254, False), (255, 255, True),
             (256, 255, False), (638, 638, True), (639, 639, True), (639, 638, False), (1000, 1000, False)]
FIX_IDS = [f"L{L}_M{M}_{'f32' if f32 else 'f64'}" for L, M, f32 in FIX_CASES]
FIX_KINDS = (FR.POS, FR.YAW, FR.POS | FR.YAW)


def fix_rule(L_max):
    """launch_fix restated: the dynamic LDS and whether slam_allow_full_lds is called."""
    lds = 8 * (6 * (3 + 2 * L_max) + 3)
    return dict(lds=lds, full_lds=lds + 4096 > 64 * 1024)


# ---- 1. association ----------------------------------------------------------------------------------------------------------------------------
# assoc_cost_phase (assoc_kernel.h) walks the slots 64 lanes at a time and joins each trip's (best, second, slot, nu) into the running values,
# an earlier trip keeping a tie.  Landmark counts around one, two and sixteen trips:
ASSOC_COUNTS = (63, 64, 65, 127, 128, 129, 1000)
ASSOC_ROLES = ("tie", "near", "lone last lane", "lone first lane", "near")
# L_max -> the landmark counts of the five instances of its handle (one past a workgroup of four wavefronts); the instances of the roles
# tie and near hold every count once in a full handle and once in a handle with room for one more (999 stands in below the capacity)
ASSOC_HANDLES = {63: (63, 62, 63, 63, 63), 64: (64, 63, 64, 64, 33), 65: (65, 64, 65, 65, 63), 66: (65, 64, 65, 65, 1),
                 127: (127, 65, 127, 127, 64), 128: (128, 127, 128, 128, 64), 129: (129, 128, 129, 129, 64), 130: (129, 65, 128, 129, 130),
                 201: (129, 128, 129, 129, 200), 1000: (1000, 999, 1000, 1000, 129)}
STEP_BEHIND = (129, 201)                                 # step class 403 and the streamed kernel: the associated step against the plain step
ASSOC_CASES = [(L, f32) for L in sorted(ASSOC_HANDLES) if L < CAPACITY for f32 in (False, True)] + [(1000, True)]
ASSOC_IDS = [f"L{L}_{'f32' if f32 else 'f64'}" for L, f32 in ASSOC_CASES]
ASSOC_TICK2 = (0, 1, 64, 65, 64)                         # the message lengths of the second tick: 65 is one too long (TOO_LONG)
NEAR = 0.06                                              # metres between the two slots of a near pair: 1.2 sigma of the range noise


def trip(slot):
    return slot // 64


def assoc_slots(role, M):
    """The slots a role is built around.  tie: (lower, upper) hold identical x entries and identical blocks of P, in the first and the
    last trip; near: (early, late), late = M - 1 in the last trip lies NEAR metres behind early in the first; lone: the only slot whose
    cost is finite, the last lane of a trip (127, 63) or the first of the next (128, 64) where the map reaches it."""
    last0 = 64 * ((M - 1) // 64)                         # the first slot of the last trip
    if role == "tie":
        return (2, last0) if last0 else (2, M - 1)
    if role == "near":
        return (min(7, M - 2), M - 1) if M > 1 else (0, 0)
    if role == "lone last lane":
        return (next((s for s in (127, 63) if s < M), M - 1),)
    return (next((s for s in (128, 64) if s < M), 0),)


def assoc_state(role, M, f32, rng):
    """assoc_reference.grid_state with the role's slots crafted into it."""
    import assoc_reference as AR
    st = AR.grid_state(rng, M, f32)
    x, P = st["x"].copy(), st["P"].copy()
    sl = assoc_slots(role, M)
    if role == "tie":
        a, b = (3 + 2 * s for s in sl)
        x[b:b + 2] = x[a:a + 2]
        P[b:b + 2, :3] = P[a:a + 2, :3]; P[:3, b:b + 2] = P[:3, a:a + 2]; P[b:b + 2, b:b + 2] = P[a:a + 2, a:a + 2]
    elif role == "near" and M > 1:
        a, b = (3 + 2 * s for s in sl)
        d = x[a:a + 2] - x[:2]
        x[b:b + 2] = x[a:a + 2] + NEAR * d / np.hypot(*d)
    elif role.startswith("lone"):
        keep = 3 + 2 * sl[0]
        lm = x[keep:keep + 2].copy()
        x[3:] = np.nan
        x[keep:keep + 2] = lm
    st = dict(st, x=R.as_stored(x, f32), P=R.as_stored(P, f32))
    return st


def assoc_messages(role, st, rng, k=None):
    """The triplets of one instance.  k None: the detections the role is about - the exact view of each of its slots
    (joint_reference.seen), something new, two clean detections.  Else a message of k detections (the second tick: ASSOC_TICK2)."""
    import assoc_reference as AR
    import joint_reference as JR
    M = st["M"]
    sl = assoc_slots(role, M)
    if k is None:
        m = [JR.seen(st, s) for s in sl] + [AR.fresh(3)]
        if not role.startswith("lone") and M > 12:
            m += [AR.clean(rng, st, 11), AR.clean(rng, st, M - 2)]
        return m
    if role.startswith("lone"):
        return [JR.seen(st, sl[0]) if l % 2 == 0 else AR.fresh(l) for l in range(k)]
    return [AR.clean(rng, st, (l * 13) % M) if l % 5 else AR.fresh(l) for l in range(k)]


# ---- 2. gate and innovation at the capacity ---------------------------------------------------------------------------------------------------
FILTER_MORE = (127, 128, 300, 511, 512, 700, 767, 768, 900, 960, 5, 9, 13, 17, 21, 25, 29, 37, 41, 45, 49, 53)
FILTER_ONE_MORE = 33
# L_max -> the landmark counts of the handle's instances (a frozen one rides along): the capacity, and the two handles whose gated step is
# compared with the plain step (STEP_BEHIND: step class 403 and the streamed kernel)
FILTER_HANDLES = {129: (129, 128, 129), 201: (200, 129, 201), 1000: (1000, 999, 1000)}


def filter_slots(M):
    """(the first and the last two slots and both sides of the first 64-slot boundary: 0, 63, 64, 998, 999 at the capacity; eleven more,
    SLAM_INNOV_MAX_LM = 16 distinct landmarks in all)"""
    first = (0, 63, 64, M - 2, M - 1)
    more = tuple(s for s in FILTER_MORE if s < M - 2 and s not in first)[:11]
    assert len(set(first + more)) == 16 and FILTER_ONE_MORE not in first + more
    return first, more


def filter_messages(rng, st):
    """[(name, triplets with ids, gate verdicts or None, flags)] on a state of at least 128 landmarks: clean detections
    (innovation_reference.detection) and range spikes of 1 m (gate_reference.spiked)."""
    import gate_reference as GR
    import innovation_reference as IR
    A, Rj, N = GR.ACCEPTED, GR.REJECTED, GR.NONE
    det = lambda s: IR.detection(rng, st, s)
    M = st["M"]
    first, more = filter_slots(M)
    sixteen = first + more
    return [("the first and last slots and the first trip boundary", [det(0), det(63), GR.spiked(det(64)), det(M - 2), GR.spiked(det(M - 1))],
             [A, A, Rj, A, Rj], 0),
            ("exactly MAX_LM distinct landmarks", [GR.spiked(det(s)) if s in (64, more[-1]) else det(s) for s in sixteen],
             [Rj if s in (64, more[-1]) else A for s in sixteen], 0),
            ("one more than MAX_LM distinct landmarks", [det(s) for s in sixteen + (FILTER_ONE_MORE,)], None, IR.TOO_LONG),
            ("the last slot twice, the first spiked, and a new id", [GR.spiked(det(M - 1)), det(M - 1), IR.detection(rng, st, new_id=7), det(0)],
             [Rj, A, N, A], 0)]


# ---- 1. (joint) joint-compatibility association -------------------------------------------------------------------------------------------------
# joint_kernel.h shares assoc_cost_phase and keeps kJointMaxCand = 4 candidates per detection, inserted trip by trip.  A tie of the two
# BEST costs has two equally good hypotheses, which joint_reference's margins (the best hypothesis 1e-9 from the runner-up) rule out:
# that tie is run by slam_associate alone.  A tie of the fourth and fifth best costs is run here (cluster_tie).
JOINT_ROLES = ("near", "cluster", "lone")
# L_max -> the landmark counts of the three instances (one past a workgroup of two); near and cluster hold every count full and one below
JOINT_HANDLES = {63: (63, 62, 63), 64: (63, 64, 64), 65: (64, 65, 65), 66: (65, 65, 64), 127: (127, 65, 127), 128: (127, 128, 128),
                 129: (128, 129, 129), 130: (129, 129, 65), 201: (128, 200, 129), 1000: (999, 1000, 1000)}
JOINT_CASES = [(L, f32) for L in sorted(JOINT_HANDLES) if L < CAPACITY for f32 in (False, True)] + [(1000, False)]
JOINT_IDS = [f"L{L}_{'f32' if f32 else 'f64'}" for L, f32 in JOINT_CASES]
JOINT_TICK2 = (0, 64, 65)
CLUSTER = {6: (0.06, 0.10, 0.14, 0.03, 0.10, 0.0), 5: (0.06, 0.10, 0.10, 0.03, 0.0)}     # metres behind the last slot of the cluster


def joint_role(role, L_max):
    """The lone slot is a trip's last lane in the handles of even L_max and the first lane of the next trip in the others."""
    return role if role != "lone" else ("lone last lane" if L_max % 2 == 0 else "lone first lane")


def cluster_slots(M):
    """Five or six slots within a few centimetres of each other, over three trips where the map has them: more than kJointMaxCand = 4
    landmarks inside the individual gate of a detection of the last one."""
    if M >= 130:
        return (3, 40, 70, 100, 128, M - 1)
    if M == 129:
        return (3, 20, 40, 70, 100, 128)
    if M > 101:
        return (3, 20, 40, 70, 100, M - 1)
    return (3, 20, 40, 55, M - 1)


def cluster_tie(M):
    """(lower, upper): the two slots of the cluster whose costs are the same bits and rank fourth and fifth, so that JointSink::pair's
    insertion rule alone ("entries already there have lower j: they stay in front on a tie", joint_kernel.h) decides which is kept - in
    different trips where the cluster has six slots.  The best hypothesis and its margin do not involve them."""
    sl = cluster_slots(M)
    return (sl[1], sl[4]) if len(sl) == 6 else (sl[1], sl[2])


def joint_state(role, M, f32, rng):
    import assoc_reference as AR
    if role != "cluster":
        return assoc_state(role, M, f32, rng)
    st = AR.grid_state(rng, M, f32)
    x = st["x"].copy()
    sl = cluster_slots(M)
    base = x[3 + 2 * sl[-1]:5 + 2 * sl[-1]].copy()
    d = (base - x[:2]) / np.hypot(*(base - x[:2]))
    for s, off in zip(sl, CLUSTER[len(sl)]):
        x[3 + 2 * s:5 + 2 * s] = base + off * d
    P = st["P"].copy()
    a, b = (3 + 2 * s for s in cluster_tie(M))             # the fourth and fifth best: identical x entries and blocks of P
    x[b:b + 2] = x[a:a + 2]
    P[b:b + 2, :3] = P[a:a + 2, :3]; P[:3, b:b + 2] = P[:3, a:a + 2]; P[b:b + 2, b:b + 2] = P[a:a + 2, a:a + 2]
    return dict(st, x=R.as_stored(x, f32), P=R.as_stored(P, f32))


def joint_messages(role, st, rng, k=None):
    import assoc_reference as AR
    import joint_reference as JR
    if role != "cluster":
        return assoc_messages(role, st, rng, k)[:1 if (k is None and role.startswith("lone")) else None]     # (the lone instance: k = 1)
    M = st["M"]
    if k is None:
        return [JR.seen(st, cluster_slots(M)[-1]), AR.clean(rng, st, 11), AR.fresh(3)]
    return [AR.clean(rng, st, (l * 13) % M) if l % 5 else AR.fresh(l) for l in range(k)]
