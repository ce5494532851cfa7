// The device HashList (hash-list-inl.h:39-54 Clear, :129-174 Insert) shared by the order-faithful decoders (k2_viterbi_faithful and
// k2_lattice_faster): one Elem per key in `pool`; the list is "buckets in order of first occupation, insertion order inside a
// bucket"; b_last / b_prev per bucket (-1: empty / none).  Insert is find-or-insert: a new Elem gets its key and list link, the
// caller fills the payload.  hash_size is SetSize's; the caller grows it (PossiblyResizeHash) only while the list is empty.
template <class Elem>
struct K2HashList {
  Elem* pool;
  int pool_n;
  size_t hash_size;
  int32_t* b_last;
  int32_t* b_prev;
  int list_head, bucket_tail;
  __device__ void init(int nbuckets) {
    for (int i = 0; i < nbuckets; ++i) b_last[i] = -1;
    list_head = -1; bucket_tail = -1;
  }
  __device__ int insert(int key, bool* is_new) {
    const size_t index = (size_t)key % hash_size;
    if (b_last[index] >= 0) {
      const int head = (b_prev[index] < 0) ? list_head : pool[b_last[b_prev[index]]].tail;
      const int tail = pool[b_last[index]].tail;
      for (int e = head; e != tail; e = pool[e].tail)
        if (pool[e].key == key) { *is_new = false; return e; }
    }
    const int e = pool_n++;
    pool[e].key = key;
    if (b_last[index] < 0) {
      if (bucket_tail < 0) list_head = e; else pool[b_last[bucket_tail]].tail = e;
      pool[e].tail = -1;
      b_last[index] = e; b_prev[index] = bucket_tail; bucket_tail = (int)index;
    } else {
      pool[e].tail = pool[b_last[index]].tail;
      pool[b_last[index]].tail = e;
      b_last[index] = e;
    }
    *is_new = true;
    return e;
  }
  __device__ int clear() {          // detach the list, empty the buckets
    for (int b = bucket_tail; b >= 0; b = b_prev[b]) b_last[b] = -1;
    bucket_tail = -1;
    const int h = list_head;
    list_head = -1;
    return h;
  }
};
