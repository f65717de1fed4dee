// fl_halo.hip -- every ghost exchange of a handle: the message plan, the one-layer exchange (fl_fill_ghosts), its overlapped form behind the
// update kernels of the CG drivers (fl_exchange_*_begin / _end), the extended-face exchanges (fl_fill_ghosts_full, _deep) and the high face
// planes of fl_poisson_rhs.  The transports themselves are in fl_comm.hip.
#include "fl_handle.h"

// The message plan of a ghost exchange of the handle: fl_halo_plan, and with `self` the self-messages of the loopback mode behind it (one
// rank, periodic axes: both faces go to this very rank, same order as the two-rank periodic case).  Returns the number of messages.
int fl_halo_messages(const fl_poisson *h, bool self, fl_halo_msg plan[12])
{
  int periodic[3];
  for (int d = 0; d < 3; ++d) periodic[d] = h->ax[d].periodic;
  int np = fl_halo_plan(&h->dec, periodic, plan);
  if (self && h->loopback)
    for (int ax = 0; ax < 3; ++ax)
      if (periodic[ax]) {
        plan[np++] = {0, 2 * ax + 1, 2 * ax, 2 * ax + 1, 2 * ax + 1};
        plan[np++] = {0, 2 * ax, 2 * ax + 1, 2 * ax, 2 * ax};
      }
  return np;
}

static int ensure_facebufs(fl_poisson *h)
{
  for (int b = 0; b < 6; ++b) {
    if (h->nbr[b] < 0 || h->wrap_local[b / 2] || h->fsend[b]) continue;
    const size_t n = (size_t)fl_plane_size(h, b / 2);
    FL_CHK(fl_dev_alloc(h, (void **)&h->fsend[b], sizeof(double) * n, true));
    FL_CHK(fl_dev_alloc(h, (void **)&h->frecv[b], sizeof(double) * n, true));
  }
  return 0;
}

// the messages of one ghost exchange (the plan with its loopback self-messages) and the buffers they use
static int halo_messages(fl_poisson *h, std::vector<Msg> &msgs, double *sbuf[6], double *rbuf[6])
{
  FL_CHK(ensure_facebufs(h));
  fl_halo_msg plan[12];
  const int   np = fl_halo_messages(h, true, plan);
  for (int b = 0; b < 6; ++b) sbuf[b] = rbuf[b] = nullptr;
  for (int a = 0; a < np; ++a) {
    const int sb = plan[a].send_boundary, rb = plan[a].recv_boundary;
    sbuf[sb] = h->fsend[sb];
    rbuf[rb] = h->frecv[rb];
    msgs.push_back({plan[a].peer, h->fsend[sb], h->frecv[rb], (int64_t)fl_plane_size(h, sb / 2), plan[a].sendtag, plan[a].recvtag});
  }
  return 0;
}

// ghosts of a padded vector: local periodic images + neighbour ranks' boundary cells (DMGlobalToLocal of the reference)
int fl_fill_ghosts(fl_poisson *h, double *v)
{
  const GridP &g = h->g;
  for (int d = 0; d < 3; ++d)
    if (h->wrap_local[d]) launch_wrap(h->stream, g, v, d);
  if (!h->multi) return 0;
  if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  std::vector<Msg> msgs;
  double          *sbuf[6], *rbuf[6];
  FL_CHK(halo_messages(h, msgs, sbuf, rbuf));
  if (!msgs.empty()) launch_pack_faces(h->stream, g, v, sbuf);    // all boundary layers in one launch
  FL_CHK(h->comm.exchange(h->stream, msgs));
  if (!msgs.empty()) launch_unpack_faces(h->stream, g, v, rbuf);  // all ghost layers in one launch
  return 0;
}

// staging buffers of the extended-face exchanges: two layers of the largest face with two cells of extension on every side
static int ensure_xbufs(fl_poisson *h, int sb, int rb)
{
  const GridP &g = h->g;
  const size_t cap = 2 * (size_t)(std::max(g.nx, g.ny) + 4) * (size_t)(std::max(g.ny, g.nz) + 4);
  for (int bnd : {sb, rb}) {
    if (bnd < 0 || h->xsend[bnd]) continue;
    FL_CHK(fl_dev_alloc(h, (void **)&h->xsend[bnd], sizeof(double) * cap, true));
    FL_CHK(fl_dev_alloc(h, (void **)&h->xrecv[bnd], sizeof(double) * cap, true));
  }
  h->xcap = cap;
  return 0;
}

// One axis of an extended-face exchange: the messages of the plan that leave along axis d, `layers` layers each of the face extended by the
// ea / eb ghost layers its in-face directions hold already; face(buf, side, mode) packs (mode 1) or unpacks (mode 2) one side.  The sides
// that received are unpacked.  *sent: whether the axis had a message at all.
template <class Face>
static int exchange_axis(fl_poisson *h, const fl_halo_msg *plan, int np, int d, int ea, int eb, int layers, int tag, Face &&face, bool *sent)
{
  const GridP     &g   = h->g;
  const int64_t    cnt = layers * (int64_t)((d == 0 ? g.ny : g.nx) + 2 * ea) * ((d == 2 ? g.ny : g.nz) + 2 * eb);
  std::vector<Msg> msgs;
  bool             recv_side[2] = {false, false};
  for (int a = 0; a < np; ++a) {
    const int sb = plan[a].send_boundary, rb = plan[a].recv_boundary;
    if (sb / 2 != d) continue;
    FL_CHK(ensure_xbufs(h, sb, rb));
    face(h->xsend[sb], sb % 2, 1);
    msgs.push_back({plan[a].peer, h->xsend[sb], h->xrecv[rb], cnt, plan[a].sendtag + tag, plan[a].recvtag + tag});
    recv_side[rb % 2] = true;
  }
  *sent = !msgs.empty();
  FL_CHK(h->comm.exchange(h->stream, msgs));  // no message: returns at once
  for (int side = 0; side < 2; ++side)
    if (recv_side[side]) face(h->xrecv[2 * d + side], side, 2);
  return 0;
}

// Ghost layers INCLUDING the edge and corner cells (what a 27-point footprint reads: the tri-linear prolongation of the multigrid cycle):
// the axes are handled one after the other, and the face exchanged / wrapped along axis d spans the ghost layers the axes before it
// have already filled, so that an edge cell arrives in two hops and a corner cell in three -- the reference's DMStag would do the same
// with DMSTAG_STENCIL_BOX.  Three exchanges instead of one; used on coarse correction vectors only.
int fl_fill_ghosts_full(fl_poisson *h, double *v)
{
  const GridP &g = h->g;
  if (h->multi && h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  fl_halo_msg plan[12];
  const int   np = h->multi ? fl_halo_messages(h, true, plan) : 0;
  for (int d = 0; d < 3; ++d) {
    const int ea = d >= 1 ? 1 : 0, eb = d >= 2 ? 1 : 0;  // in-face directions: (y, z), (x, z), (x, y)
    if (h->wrap_local[d]) {
      launch_face_ext(h->stream, g, v, nullptr, d, 0, ea, eb, 0);
      continue;
    }
    if (!h->multi) continue;
    bool sent;
    FL_CHK(exchange_axis(h, plan, np, d, ea, eb, 1, 64, [&](double *buf, int side, int mode) { launch_face_ext(h->stream, g, v, buf, d, side, ea, eb, mode); }, &sent));
  }
  return 0;
}

// TWO ghost layers across every boundary behind which a neighbouring rank sits, edge and corner cells of that shell included (the reference's
// DMStag has stencil width 1, cart.c:66: this layer is a build-side extension): what two fused stencil steps read (k_cheb2: x at distance two
// along an axis and at the diagonal neighbours in a plane).  Dimension by dimension like fl_fill_ghosts_full: the two layers sent along axis d
// span the ghost layers the axes before it have received.  Axes held by one rank are left alone (a periodic one wraps inside the block, and
// the kernel wraps its indices there; behind a wall there is nothing).  Needs the wide layout (h->gw == 2).
int fl_fill_ghosts_deep(fl_poisson *h, double *v)
{
  const GridP &g = h->g;
  if (!h->multi) return 0;
  if (h->gw < 2) return FL_ERR_ARG_WRONGSTATE;
  if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  fl_halo_msg plan[12];
  const int   np = fl_halo_messages(h, false, plan);  // no loopback self-messages: the kernels that read two layers refuse the loopback mode (fl_cheb2_usable)
  int         ext[3] = {0, 0, 0};  // ghost layers axis d holds once it has been handled
  for (int d = 0; d < 3; ++d) {
    const int a1 = d == 0 ? 1 : 0, a2 = d == 2 ? 1 : 2;  // in-face directions: (y, z), (x, z), (x, y)
    const int ea = ext[a1], eb = ext[a2];
    bool      sent;
    FL_CHK(exchange_axis(h, plan, np, d, ea, eb, 2, 128, [&](double *buf, int side, int mode) { launch_face_ext_deep(h->stream, g, v, buf, d, side, ea, eb, 2, mode); }, &sent));
    if (sent) ext[d] = 2;  // an axis without a message is skipped
  }
  return 0;
}

// The overlapped exchange of the CG drivers: the boundary layers are packed on the handle's stream (pack(sbuf)); a second stream waits for the
// pack, runs the transfers and writes the ghost layers of dst.  That stream and the two events that order it are created by the first call.
template <class Pack>
static int exchange_begin(fl_poisson *h, Pack &&pack, double *dst)
{
  if (!h->multi) return 0;
  if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  if (!h->comm_stream) {
    FL_HIP(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    FL_HIP(hipEventCreateWithFlags(&h->ev_packed, hipEventDisableTiming));
    FL_HIP(hipEventCreateWithFlags(&h->ev_ghosts, hipEventDisableTiming));
  }
  std::vector<Msg> msgs;
  double          *sbuf[6], *rbuf[6];
  FL_CHK(halo_messages(h, msgs, sbuf, rbuf));
  if (!msgs.empty()) pack(sbuf);
  FL_HIP(hipEventRecord(h->ev_packed, h->stream));
  FL_HIP(hipStreamWaitEvent(h->comm_stream, h->ev_packed, 0));
  FL_CHK(h->comm.exchange(h->comm_stream, msgs));
  if (!msgs.empty()) launch_unpack_faces(h->comm_stream, h->g, dst, rbuf);
  FL_HIP(hipEventRecord(h->ev_ghosts, h->comm_stream));
  return 0;
}

// The CG iteration's ghost exchange of r, hidden behind k_cg_Bq (the DMGlobalToLocalBegin / ...End pair of the reference,
// fdapply.c:71, cnlinearcart3d.c:893-894).  begin: the boundary layers of r - alpha q are packed on the handle's stream BEFORE
// k_cg_Bq forms the new r; a second stream waits for the pack, runs the transfers and writes the ghost layers, which k_cg_Bq neither
// reads nor writes.  end: the handle's stream waits for the ghosts (and fills the locally wrapped axes) before k_cg_A needs them.
int fl_exchange_r_begin(fl_poisson *h, double *r, const double *q)  // q: valid on the boundary layers of the block at least (PlanA::qb)
{
  return exchange_begin(h, [&](double *const sbuf[6]) { launch_pack_faces_rq(h->stream, h->g, r, q, h->scal, sbuf); }, r);
}

// The single-reduction CG's exchange behind its update kernel (MODE 10): the boundary layers of the new residual are packed from r, the kept S and W
// (k_pack_faces_sr) on the handle's stream, a second stream runs the transfers and writes the ghost layers of rn -- the buffer MODE 10 fills with the
// new residual's owned cells meanwhile.  fl_exchange_r_end(h, rn) closes it.
int fl_exchange_sr_begin(fl_poisson *h, const double *r, const double *sb, const double *W, double *rn)
{
  return exchange_begin(h, [&](double *const sbuf[6]) { launch_pack_faces_sr(h->stream, h->g, r, sb, W, h->scal, sbuf); }, rn);
}
int fl_exchange_r_end(fl_poisson *h, double *r)
{
  for (int d = 0; d < 3; ++d)
    if (h->wrap_local[d]) launch_wrap(h->stream, h->g, r, d);
  if (!h->multi) return 0;
  FL_HIP(hipStreamWaitEvent(h->stream, h->ev_ghosts, 0));
  return 0;
}

bool fl_any_ghost_exchange(const fl_poisson *h) { return h->multi || h->wrap_local[0] || h->wrap_local[1] || h->wrap_local[2]; }

// fl_poisson_rhs: the high face of a rank's last owned cells along an axis belongs to the next rank (or is the periodic image of face 0).
// Fills h->hiface[d] for every axis whose high boundary face this rank does not own.
int fl_fill_hifaces(fl_poisson *h, const double *const V[3])
{
  const GridP &g = h->g;
  for (int d = 0; d < 3; ++d) {
    const int len = d == 0 ? g.nx : (d == 1 ? g.ny : g.nz);
    if ((d == 0 ? g.fx : (d == 1 ? g.fy : g.fz)) > len) continue;  // this rank owns its high boundary face
    const size_t n = (size_t)fl_plane_size(h, d);
    if (!h->hiface[d]) FL_CHK(fl_dev_alloc(h, (void **)&h->hiface[d], sizeof(double) * n, true));
    if (h->wrap_local[d]) launch_face_plane0(h->stream, g, V[d], h->hiface[d], d);
    else if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  }
  if (!h->multi) return 0;
  // every rank with a low neighbour ships its first face plane there (send only); every rank with a high neighbour
  // receives that plane as the high face of its last cells (receive only)
  std::vector<Msg> msgs;
  for (int d = 0; d < 3; ++d) {
    if (h->wrap_local[d]) continue;
    const int     lo = h->nbr[2 * d], hi = h->nbr[2 * d + 1];
    const int64_t n  = fl_plane_size(h, d);
    if (lo >= 0) {
      if (!h->loface_send[d]) FL_CHK(fl_dev_alloc(h, (void **)&h->loface_send[d], sizeof(double) * n, true));
      launch_face_plane0(h->stream, g, V[d], h->loface_send[d], d);
    }
    if (lo >= 0 && lo == hi) {
      msgs.push_back({lo, h->loface_send[d], h->hiface[d], n, 6 + d, 6 + d});
    } else {
      if (lo >= 0) msgs.push_back({lo, h->loface_send[d], nullptr, n, 6 + d, 6 + d});
      if (hi >= 0) msgs.push_back({hi, nullptr, h->hiface[d], n, 6 + d, 6 + d});
    }
  }
  return h->comm.exchange(h->stream, msgs);
}
