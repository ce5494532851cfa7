"""Kaldi's `Posterior` of a batch as flat arrays and back: what `DevicePosteriors.from_arrays` uploads and
`DevicePosteriors.download_arrays` / `frame_off` give back.

A Posterior is, per frame, a list of (transition-id, weight); `posts[u][t]` is that list for frame t of utterance u.  The arrays:
frame_off [n_utt + 1] (utterance u owns frames frame_off[u] .. frame_off[u + 1]), entry_begin [frames + 1] (frame f owns entries
entry_begin[f] .. entry_begin[f + 1]), tid int32 / weight float64 [entries]."""
from typing import List, Sequence, Tuple

import numpy as np

Posterior = List[List[Tuple[int, float]]]


def ali_to_post(ali: Sequence[int]) -> Posterior:
    """ali-to-post: every frame's transition-id with weight 1.0."""
    return [[(int(t), 1.0)] for t in ali]


def posts_to_arrays(posts: Sequence[Posterior]):
    """-> (frame_off, entry_begin, tid, weight)."""
    frame_off = np.zeros(len(posts) + 1, np.int64)
    counts, tid, weight = [], [], []
    for u, post in enumerate(posts):
        frame_off[u + 1] = frame_off[u] + len(post)
        for frame in post:
            counts.append(len(frame))
            for t, w in frame:
                tid.append(int(t))
                weight.append(float(w))
    entry_begin = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=entry_begin[1:])
    return frame_off, entry_begin, np.asarray(tid, np.int32), np.asarray(weight, np.float64)


def arrays_to_posts(frame_off, entry_begin, tid, weight) -> List[Posterior]:
    """The inverse of posts_to_arrays."""
    posts = []
    for u in range(len(frame_off) - 1):
        post = []
        for f in range(int(frame_off[u]), int(frame_off[u + 1])):
            post.append([(int(tid[e]), float(weight[e])) for e in range(int(entry_begin[f]), int(entry_begin[f + 1]))])
        posts.append(post)
    return posts
