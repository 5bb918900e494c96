"""The consistent-group bookkeeping of ORB-SLAM2's LoopClosing::DetectLoop, restated on keyframe serials.  Pure Python: the
candidates and their groups come from LocalMapper.loop_candidates (mo_map_loop_candidates); this file only remembers, from one asking
keyframe to the next, which groups of keyframes were candidates before.

A group is the set of serials of a candidate keyframe and the keyframes connected to it.  A keyframe position cannot name a keyframe
across calls (positions are renumbered after every keyframe cull), so groups hold creation serials; the serial of a keyframe that was
removed since simply never turns up in a new group again."""


class LoopConsistency:
    def __init__(self, threshold=3):
        self.threshold = int(threshold)
        self.groups = []   # [(frozenset of serials, count)] of the last call

    def reset(self):
        self.groups = []

    def update(self, candidates):
        """candidates: [(candidate serial, iterable of group serials)] of one asking keyframe, in order.  Returns
        (reported, consistency): the serials of the candidates whose consistency reached the threshold, in order, each once; and per
        candidate the largest consistency it reached (0: consistent with no previous group).
        For each candidate and each previous group that shares a serial with the candidate's group: the candidate's consistency is that
        group's count + 1, and (candidate group, count + 1) joins the new state - once per previous group per call.  A candidate
        consistent with no previous group joins the new state with count 0.  The new state replaces the old one; an empty candidate list
        clears it."""
        new, reported, consistency = [], [], []
        taken = [False] * len(self.groups)
        for serial, group in candidates:
            group = frozenset(group)
            enough = consistent_with_some = False
            top = 0
            for i, (prev, count) in enumerate(self.groups):
                if not (group & prev):
                    continue
                consistent_with_some = True
                now = count + 1
                top = max(top, now)
                if not taken[i]:
                    new.append((group, now))
                    taken[i] = True
                if now >= self.threshold and not enough:
                    reported.append(serial)
                    enough = True
            if not consistent_with_some:
                new.append((group, 0))
            consistency.append(top)
        self.groups = new
        return reported, consistency
