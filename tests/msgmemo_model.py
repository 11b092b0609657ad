"""A dictionary model of the hash-point memo's index (teku_amd/csrc/tb_msgmemo.h),
written from the stated rules and not from the code under test; shared by
tests/test_msgmemo_host.py (against the header itself) and the GPU tests
(against the library's counters).

Rules: messages of up to 64 bytes are cacheable; a shard's distinct messages
are taken in first-appearance order; `new` counts the distinct cacheable
messages that are not resident; if new <= free rows they take the next free
rows in order; otherwise the index is flushed (and the flush counted), every
distinct cacheable message of the shard is new, the first min(count, R) take
rows 0, 1, ... and the rest are hashed and not learned.  m_hash lists the
distinct messages that are not served from a row, src[g] is ROW | r or the
position in m_hash, learn[j] the row or NONE.  hits counts the pairs served
from a row: one per set in an ungrouped pass, one per distinct message in a
grouped one."""

ROW, NONE, MSG_MAX = 0x80000000, 0xFFFFFFFF, 64


class Model:
    def __init__(self, rows):
        self.rows, self.row_of = rows, {}
        self.hits = self.hashed = self.flushes = 0

    def invalidate(self):
        self.row_of = {}

    def stats(self):
        return (self.hits, self.hashed, self.flushes, len(self.row_of))

    def shard(self, msgs, per_set=True):
        distinct = list(dict.fromkeys(msgs))
        count = {}
        for m in msgs:
            count[m] = count.get(m, 0) + 1
        new = [m for m in distinct if len(m) <= MSG_MAX and m not in self.row_of]
        flushed = len(new) > self.rows - len(self.row_of)
        if flushed:
            self.row_of = {}
            self.flushes += 1
        m_hash, src, learn = [], [], []
        for g, m in enumerate(distinct):
            if m in self.row_of:
                src.append(ROW | self.row_of[m])
                self.hits += count[m] if per_set else 1
                continue
            src.append(len(m_hash))
            m_hash.append(g)
            if len(m) <= MSG_MAX and len(self.row_of) < self.rows:
                self.row_of[m] = len(self.row_of)
                learn.append(self.row_of[m])
            else:
                learn.append(NONE)
        self.hashed += len(m_hash)
        return dict(m_hash=m_hash, src=src, learn=learn, flushed=int(flushed), hits=self.hits, hashed=self.hashed, flushes=self.flushes,
                    used=len(self.row_of))
