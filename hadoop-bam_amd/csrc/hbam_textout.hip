// hbam_textout.hip — what the text writers share on the host: hbam_sam_render (hbam_samtext.hip),
// hbam_vcf_render (hbam_vcftext.hip) and hbam_frag_render (hbam_fragtext.hip) are one sequence with
// their own kernels between its steps.  Included in hbam_capi.hip before the three.
//   stage_records    host records + 64 zero bytes and their offsets into context buffers
//   textout_begin    the per-line arrays, first_stop armed (textout_arm), event 0
//   textout_stop     after a pass that can stop (atomicMin(first_stop) at a bad line): the lines
//                    before it stand; the caller sets the status and, after textout_layout, cuts
//                    text_len and n_def
//   textout_layout   len -> line_off, text_len; dflag -> dpos, n_def, deferred; the text; event 1
//   textout_finish   the result; walk_ms = sizes + scans, huffman_ms and resolve_ms = the write passes

namespace hbam {

constexpr uint32_t TEXTOUT_WG = 256;

// the output positions of the deferred lines, ascending (dpos = the exclusive scan of dflag)
__global__ __launch_bounds__(TEXTOUT_WG) void k_text_deferred(const uint32_t* __restrict__ dflag,
                                                              const uint64_t* __restrict__ dpos, uint32_t n,
                                                              uint32_t* __restrict__ deferred) {
  const uint32_t k = blockIdx.x * TEXTOUT_WG + threadIdx.x;
  if (k < n && dflag[k]) deferred[dpos[k]] = k;
}

}  // namespace hbam

namespace {

struct TextOut {
  // The format's own buffers: a render's text, line_off and deferred survive a later render of
  // another format on the same context.  deferral: dflag, dpos and deferred exist.
  struct Ids {
    BufId len, status, line_off, small, text;
    bool deferral;
    BufId dflag, dpos, deferred;
  } ids;
  uint32_t *len, *dflag = nullptr, *deferred = nullptr;
  int32_t* lstatus;  // per line; the format's own meaning (hbam_fragtext.hip keeps flag bits here)
  uint64_t *line_off, *dpos = nullptr;
  unsigned long long* first_stop;
  uint8_t* text = nullptr;
  uint64_t m;  // the host's results: the lines that stand (cut: textout_stop lowered it), ...
  bool cut = false;
  int32_t status = HBAM_OK;
  uint64_t text_len = 0, n_def = 0;
};

int stage_records(hbam_ctx* c, BufId id_bytes, BufId id_off, const uint8_t* bytes, uint64_t n_bytes,
                  const uint64_t* rec_off, uint64_t n_off, const uint8_t** ub, const uint64_t** ro) {
  int rc;
  uint8_t* dub;
  uint64_t* dro;
  if ((rc = ensure(c, id_bytes, n_bytes + 64, &dub)) || (rc = ensure(c, id_off, n_off, &dro))) return rc;
  if (n_bytes) HIPCHK(c, hipMemcpyAsync(dub, bytes, n_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(dub + n_bytes, 0, 64, c->stream));
  HIPCHK(c, hipMemcpyAsync(dro, rec_off, n_off * 8, hipMemcpyHostToDevice, c->stream));
  *ub = dub, *ro = dro;
  return HBAM_OK;
}

// no line has stopped the output
int textout_arm(hbam_ctx* c, const TextOut& T) {
  HIPCHK(c, hipMemsetAsync(T.first_stop, 0xff, 8, c->stream));
  return HBAM_OK;
}

int textout_begin(hbam_ctx* c, uint64_t n, TextOut* T) {
  const TextOut::Ids& ids = T->ids;
  int rc;
  uint64_t* small;
  T->m = n;
  if ((rc = ensure(c, ids.len, n + 1, &T->len)) || (rc = ensure(c, ids.status, n + 1, &T->lstatus)) ||
      (rc = ensure(c, ids.line_off, n + 1, &T->line_off)) || (rc = ensure(c, ids.small, 2, &small)))
    return rc;
  if (ids.deferral && ((rc = ensure(c, ids.dflag, n + 1, &T->dflag)) || (rc = ensure(c, ids.dpos, n + 1, &T->dpos)) ||
                       (rc = ensure(c, ids.deferred, n + 1, &T->deferred))))
    return rc;
  T->first_stop = (unsigned long long*)small;
  if ((rc = textout_arm(c, *T))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  return HBAM_OK;
}

// One round trip.  cut: a line below m stopped the output; m is now that line.
int textout_stop(hbam_ctx* c, TextOut* T) {
  HIPCHK(c, hipMemcpyAsync(c->pinned_small + 8, T->first_stop, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T->cut = c->pinned_small[8] < T->m;
  if (T->cut) T->m = c->pinned_small[8];
  return HBAM_OK;
}

int textout_layout(hbam_ctx* c, TextOut* T) {
  int rc;
  if ((rc = scan_exclusive<uint32_t>(c, T->len, T->m, T->line_off, &T->text_len))) return rc;
  if (T->ids.deferral) {
    if ((rc = scan_exclusive<uint32_t>(c, T->dflag, T->m, T->dpos, &T->n_def))) return rc;
    if (T->m)
      hbam::k_text_deferred<<<grid_for(T->m, hbam::TEXTOUT_WG), hbam::TEXTOUT_WG, 0, c->stream>>>(
          T->dflag, T->dpos, (uint32_t)T->m, T->deferred);
    HIPCHK(c, hipGetLastError());
  }
  if ((rc = ensure(c, T->ids.text, T->text_len + 64, &T->text))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  return HBAM_OK;
}

// hbam_sam_text / hbam_vcf_text or hbam_frag_text: the fields they share, and the timing
template <class Out>
void textout_finish(hbam_ctx* c, const TextOut& T, Out* out) {
  out->n_records = T.m;
  out->status = T.status;
  out->err_record = T.status ? T.m : 0;
  out->text_len = T.text_len;
  out->text = T.text;
  out->line_off = T.line_off;
  c->timing.walk_ms = ev_ms(c, 0, 1);
  c->timing.huffman_ms = ev_ms(c, 1, 2);
  c->timing.resolve_ms = ev_ms(c, 2, 3);
  c->timing.total_ms = ev_ms(c, 0, 3);
  c->timing.n_records = T.m;
  c->timing.ubuf_bytes = T.text_len;
}

}  // namespace
