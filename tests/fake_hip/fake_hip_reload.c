/* fake_hip_reload.c -- TEST INFRASTRUCTURE: the CPU stand-in of fake_hip.c (included unchanged) plus the live-reload entry points
 * of include/sayuri_hip.h (sayuri_hip_reload_begin / _prepare / _commit / _abort, sayuri_hip_weights_generation).
 *
 * fake_hip.c's network ignores its tensors.  Here every reply carries a CHECKSUM of the tensors of the weight set that was live
 * when its batch was ENQUEUED: `delta`, a number in [0, 10) derived from every loaded tensor, is added to each pass and misc
 * output of the batch.  Two networks written under two seeds have two deltas, so a test can tell network A's answer from B's for
 * every single reply, and a batch that was in flight across a commit keeps the delta of the network it was sent to.
 *
 * The entry points the stand-in shares with fake_hip.c are renamed around the include and wrapped; the state the wrappers need sits
 * beside the context in a small table (fake_hip.c's struct is not touched). */
#define sayuri_hip_create fake_base_create
#define sayuri_hip_destroy fake_base_destroy
#define sayuri_hip_load_tensor fake_base_load_tensor
#define sayuri_hip_forward fake_base_forward
#define sayuri_hip_forward_packed fake_base_forward_packed
#define sayuri_hip_submit fake_base_submit
#define sayuri_hip_submit_packed fake_base_submit_packed
#define sayuri_hip_wait fake_base_wait
#include "fake_hip.c"
#undef sayuri_hip_create
#undef sayuri_hip_destroy
#undef sayuri_hip_load_tensor
#undef sayuri_hip_forward
#undef sayuri_hip_forward_packed
#undef sayuri_hip_submit
#undef sayuri_hip_submit_packed
#undef sayuri_hip_wait

#include <math.h>

struct wset {
    double sum;  /* checksum of the tensors loaded so far */
    int tensors; /* how many */
};
struct rstate {
    sayuri_hip_ctx* c;
    sayuri_hip_netdesc desc;
    sayuri_hip_blockdesc* blocks;
    struct wset live, staged;
    int open, prepared, generation, forwarded;
    float job_delta[2]; /* per ticket: the live set's delta when the batch was enqueued */
};
#define MAX_CTX 64
static struct rstate g_rs[MAX_CTX];
static pthread_mutex_t g_rmu = PTHREAD_MUTEX_INITIALIZER; /* the table, and commit against submit */

static struct rstate* rs_of(const sayuri_hip_ctx* c) {
    for (int i = 0; i < MAX_CTX; ++i)
        if (g_rs[i].c == c) return &g_rs[i];
    return NULL;
}
static int rfail(const char* msg) {
    snprintf(g_last_error, sizeof g_last_error, "%s", msg);
    return -1;
}
static float delta_of(const struct wset* w) { return (float)(fmod(fabs(w->sum), 1000.0) * 0.01); }
static void add_tensor(struct wset* w, int layer_id, int kind, const float* host, size_t n) {
    double s = 0;
    for (size_t i = 0; i < n; ++i) s += host[i] * (double)(1 + i % 5);
    w->sum += s * (double)(1 + (2 * layer_id + kind) % 11);
    w->tensors += 1;
}
static void add_delta(const sayuri_hip_ctx* c, int n, float* pass, float* misc, float d) {
    const int PP = c->desc.pass_probability_outputs, VM = c->desc.value_misc_outputs;
    for (int i = 0; i < n * PP; ++i) pass[i] += d;
    for (int i = 0; i < n * VM; ++i) misc[i] += d;
}

sayuri_hip_ctx* sayuri_hip_create(int device, const sayuri_hip_netdesc* desc, int max_batch, int board, int use_fp16) {
    sayuri_hip_ctx* c = fake_base_create(device, desc, max_batch, board, use_fp16);
    if (!c) return NULL;
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(NULL);
    if (r) {
        memset(r, 0, sizeof *r);
        r->desc = *desc;
        r->blocks = (sayuri_hip_blockdesc*)calloc((size_t)desc->residual_blocks + 1, sizeof(sayuri_hip_blockdesc));
        memcpy(r->blocks, desc->blocks, sizeof(sayuri_hip_blockdesc) * (size_t)desc->residual_blocks);
        r->c = c;
    }
    pthread_mutex_unlock(&g_rmu);
    if (!r) {
        fake_base_destroy(c);
        rfail("fake_hip_reload: too many contexts");
        return NULL;
    }
    return c;
}
void sayuri_hip_destroy(sayuri_hip_ctx* c) {
    if (!c) return;
    fake_base_destroy(c);
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    if (r) {
        free(r->blocks);
        memset(r, 0, sizeof *r);
    }
    pthread_mutex_unlock(&g_rmu);
}

int sayuri_hip_load_tensor(sayuri_hip_ctx* c, int layer_id, int kind, const float* host, size_t n) {
    if (fake_base_load_tensor(c, layer_id, kind, host, n)) return rfail("fake_hip_reload: load_tensor: bad argument");
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    int rc = 0;
    if (!r) rc = rfail("fake_hip_reload: unknown context");
    else if (r->open && r->prepared) rc = rfail("load_tensor: the open reload is prepared already");
    else if (r->open) add_tensor(&r->staged, layer_id, kind, host, n);
    else if (r->forwarded) rc = rfail("load_tensor after the first forward");
    else add_tensor(&r->live, layer_id, kind, host, n);
    pthread_mutex_unlock(&g_rmu);
    return rc;
}

int sayuri_hip_reload_begin(sayuri_hip_ctx* c, const sayuri_hip_netdesc* d) {
    if (!c || !d) return rfail("reload_begin: null argument");
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    int rc = 0;
    if (!r) rc = rfail("fake_hip_reload: unknown context");
    else if (r->open) rc = rfail("reload_begin: a reload is already open on this context");
    else if (d->residual_blocks != r->desc.residual_blocks) rc = rfail("reload_begin: the network differs from the context's: residual_blocks");
    else if (d->residual_channels != r->desc.residual_channels) rc = rfail("reload_begin: the network differs from the context's: residual_channels");
    else if (d->input_channels != r->desc.input_channels || d->policy_head_type != r->desc.policy_head_type ||
             d->policy_head_channels != r->desc.policy_head_channels || d->value_head_channels != r->desc.value_head_channels ||
             d->default_act != r->desc.default_act)
        rc = rfail("reload_begin: the network differs from the context's: heads, inputs or activation");
    for (int b = 0; !rc && b < d->residual_blocks; ++b)
        if (d->blocks[b].type != r->blocks[b].type || d->blocks[b].apply_se != r->blocks[b].apply_se ||
            (d->blocks[b].apply_se && d->blocks[b].se_size != r->blocks[b].se_size) ||
            d->blocks[b].bottleneck_channels != r->blocks[b].bottleneck_channels ||
            d->blocks[b].feedforward_channels != r->blocks[b].feedforward_channels)
            rc = rfail("reload_begin: the network differs from the context's: a block");
    if (!rc) {
        r->open = 1;
        r->prepared = 0;
        memset(&r->staged, 0, sizeof r->staged);
    }
    pthread_mutex_unlock(&g_rmu);
    return rc;
}
int sayuri_hip_reload_prepare(sayuri_hip_ctx* c) {
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    int rc = 0;
    if (!r || !r->open) rc = rfail("reload_prepare: no reload is open");
    else if (r->prepared) rc = rfail("reload_prepare: the open reload is prepared already");
    else if (r->staged.tensors != r->live.tensors) {
        r->open = 0; /* a failed prepare closes the reload */
        rc = rfail("reload_prepare: missing tensors");
    } else r->prepared = 1;
    pthread_mutex_unlock(&g_rmu);
    return rc;
}
int sayuri_hip_reload_commit(sayuri_hip_ctx* c) {
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    int rc;
    if (!r || !r->open) rc = rfail("reload_commit: no reload is open");
    else if (!r->prepared) rc = rfail("reload_commit: the open reload is not prepared");
    else {
        r->live = r->staged;
        r->open = r->prepared = 0;
        rc = ++r->generation;
    }
    pthread_mutex_unlock(&g_rmu);
    return rc;
}
int sayuri_hip_reload_abort(sayuri_hip_ctx* c) {
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    const int rc = r && r->open ? 0 : rfail("reload_abort: no reload is open");
    if (!rc) r->open = r->prepared = 0;
    pthread_mutex_unlock(&g_rmu);
    return rc;
}
int sayuri_hip_weights_generation(const sayuri_hip_ctx* c) {
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    const int g = r ? r->generation : -1;
    pthread_mutex_unlock(&g_rmu);
    return g;
}

/* the blocking forwards: the set that is live now */
static float live_delta(sayuri_hip_ctx* c) {
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    const float d = r ? delta_of(&r->live) : 0.f;
    if (r) r->forwarded = 1;
    pthread_mutex_unlock(&g_rmu);
    return d;
}
int sayuri_hip_forward(sayuri_hip_ctx* c, int n, const float* planes, const int* bsz, float* prob, float* pass, float* misc, float* own) {
    if (fake_base_forward(c, n, planes, bsz, prob, pass, misc, own)) return -1;
    add_delta(c, n, pass, misc, live_delta(c));
    return 0;
}
int sayuri_hip_forward_packed(sayuri_hip_ctx* c, int n, const unsigned* records, int binary, const int* bsz, float* prob, float* pass,
                              float* misc, float* own) {
    if (fake_base_forward_packed(c, n, records, binary, bsz, prob, pass, misc, own)) return -1;
    add_delta(c, n, pass, misc, live_delta(c));
    return 0;
}

/* submit: the ticket remembers the delta of the set that is live NOW (a commit is serialised with this by g_rmu); the worker
 * evaluates the batch later, wait adds the remembered delta to what it wrote */
static void note_ticket(sayuri_hip_ctx* c, int ticket) {
    struct rstate* r = rs_of(c);
    if (!r) return;
    r->forwarded = 1;
    r->job_delta[ticket] = delta_of(&r->live);
}
int sayuri_hip_submit(sayuri_hip_ctx* c, int n, const float* planes, const int* bsz, float* prob, float* pass, float* misc, float* own,
                      int* ticket) {
    pthread_mutex_lock(&g_rmu);
    const int rc = fake_base_submit(c, n, planes, bsz, prob, pass, misc, own, ticket);
    if (!rc) note_ticket(c, *ticket);
    pthread_mutex_unlock(&g_rmu);
    return rc;
}
int sayuri_hip_submit_packed(sayuri_hip_ctx* c, int n, const unsigned* records, int binary, const int* bsz, float* prob, float* pass,
                             float* misc, float* own, int* ticket) {
    pthread_mutex_lock(&g_rmu);
    const int rc = fake_base_submit_packed(c, n, records, binary, bsz, prob, pass, misc, own, ticket);
    if (!rc) note_ticket(c, *ticket);
    pthread_mutex_unlock(&g_rmu);
    return rc;
}
int sayuri_hip_wait(sayuri_hip_ctx* c, int t) {
    const int rc = fake_base_wait(c, t);
    if (rc) return rc;
    pthread_mutex_lock(&g_rmu);
    struct rstate* r = rs_of(c);
    const float d = r ? r->job_delta[t] : 0.f;
    pthread_mutex_unlock(&g_rmu);
    /* (the job's buffers are its submitter's until that ticket's next submit, which comes after this wait) */
    add_delta(c, c->jobs[t].n, c->jobs[t].pass, c->jobs[t].misc, d);
    return 0;
}
