"""The plan of a dependency level (aivc_amd/codec.py: level_items, level_batches, share_level) that FrameCodec.encode_units /
decode_units and the generic drivers of aivc_amd/parallel.py walk: over the ranks of a group every frame of a level is coded
exactly once, in batches of one frame type, and the exchange puts every reconstruction back where its frame is.  No oracle,
no device, no process group: the shard is a stub with R, local and mine."""
import pytest

from aivc_amd.codec import frame_types, level_batches, level_items, share_level
from aivc_amd.func_util.GOP_structure import coding_levels, generate_gop_struct


class StubShard:
    """rank `local` of a group of R (ClipShard's R / local / mine); exchange_frames answers from `truth`, the
    reconstruction every frame is supposed to have, and checks that this rank sent exactly its own"""

    def __init__(self, R, local, truth=None):
        self.R, self.local, self.truth = R, local, truth
        self.exchanges = 0

    def mine(self, items):
        return items[self.local::self.R]

    def exchange_frames(self, items, my_recs, h, w, device):
        assert my_recs == [self.truth[it] for it in self.mine(items)]
        self.exchanges += 1
        return [self.truth[it] for it in items]


@pytest.mark.parametrize('gop_name', ['1_GOP_2', '1_GOP_4', '1_GOP_8', '1_GOP_32', 'LDP_2'])
def test_level_plan_covers_every_frame_once(gop_name):
    gop = generate_gop_struct(gop_name)
    levels = coding_levels(gop)
    assert sorted(f for level in levels for f in level) == sorted(gop)
    for n_units in (1, 2, 3):
        uids = range(n_units)
        for level in levels:
            types = frame_types(gop, level)
            every = {t: level_items(gop, level, uids, t) for t in types}
            for t in types:  # unit-major, then the level's order
                assert every[t] == [(u, f) for u in uids for f in level if gop[f]['type'] == t]
            assert sorted(it for t in types for it in every[t]) == sorted((u, f) for u in uids for f in level)
            for max_batch in (1, 3, 16):
                # without a shard: the whole level
                assert [it for _, c in level_batches(gop, level, uids, max_batch) for it in c] == [it for t in types for it in every[t]]
                for R in (1, 2, 3, 4):
                    coded = []
                    for local in range(R):
                        sh = StubShard(R, local)
                        batches = list(level_batches(gop, level, uids, max_batch, sh))
                        for t, chunk in batches:
                            assert 1 <= len(chunk) <= max_batch
                            assert all(gop[f]['type'] == t for _, f in chunk)
                        assert [t for t, _ in batches] == sorted(t for t, _ in batches)  # types in sorted order on every rank
                        for t in types:  # this rank's share, in its order, cut into batches
                            assert [it for bt, c in batches if bt == t for it in c] == sh.mine(every[t])
                        coded += [it for _, c in batches for it in c]
                    assert sorted(coded) == sorted((u, f) for u in uids for f in level)  # each frame exactly once
                    for t in types:  # what exchange_frames hands back: slot j // R of rank j % R is frame j
                        shares = [StubShard(R, local).mine(every[t]) for local in range(R)]
                        assert [shares[j % R][j // R] for j in range(len(every[t]))] == every[t]


@pytest.mark.parametrize('gop_name', ['1_GOP_4', 'LDP_2'])
def test_share_level_fills_in_the_peers_frames(gop_name):
    gop = generate_gop_struct(gop_name)
    uids = range(2)
    truth = {(u, f): 'rec %d %s' % (u, f) for u in uids for f in gop}
    for level in coding_levels(gop):
        for R in (2, 3):
            for local in range(R):
                sh = StubShard(R, local, truth)
                rec = [dict() for _ in uids]
                for _, chunk in level_batches(gop, level, uids, 3, sh):
                    for u, f in chunk:
                        rec[u][f] = truth[(u, f)]
                share_level(sh, rec, gop, level, uids, 32, 48, None)
                assert sh.exchanges == len(frame_types(gop, level))  # one collective per frame type, on every rank
                assert rec == [{f: truth[(u, f)] for f in level} for u in uids]
        # a single rank exchanges nothing (and touches neither the shard nor rec)
        alone = StubShard(1, 0)
        share_level(alone, None, gop, level, uids, 32, 48, None)
        share_level(None, None, gop, level, uids, 32, 48, None)
        assert alone.exchanges == 0
