// Stand-alone host check of the parameter-block layouts: includes the two translation units, lays out two configurations each on
// stack objects (no GPU call) and prints every (name, offset, shape) through the C ABI queries.  Host code only, so it runs under the
// host sanitizers on a machine without a GPU; built against two csrc trees (each with its built library for the symbols of the other
// units) its outputs show whether a refactor moved an offset:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I offlinerl-kit_amd/csrc \
//         tools/probes/layout_check.hip -L offlinerl-kit_amd -lorlengine -Wl,-rpath,$PWD/offlinerl-kit_amd -o tools/probes/layout_check
#include "dynamics.hip"
#include "diffusion.hip"

#include <cstdio>

static void print_row(const char* what, int i, const char* name, int64_t off, int32_t nd, const int64_t* sh) {
  printf("%s %d %s %lld [", what, i, name, (long long)off);
  for (int k = 0; k < nd; ++k) printf("%s%lld", k ? "," : "", (long long)sh[k]);
  printf("]\n");
}

static void dyn_case(int od, int ad, int nh, const int* hid, int K, int with_reward) {
  orl_dyn_config c;
  orl_dyn_config_default(&c);
  c.obs_dim = od; c.act_dim = ad; c.n_hidden = nh; c.num_ensemble = K; c.with_reward = with_reward;
  for (int i = 0; i < nh; ++i) c.hidden[i] = hid[i];
  orl_dynamics* d = new orl_dynamics();
  d->c = c;
  d->R = 1; d->K = K; d->L = nh; d->od = od; d->ad = ad; d->in = od + ad; d->D = od + (with_reward ? 1 : 0); d->O = 2 * d->D;
  d->width[0] = d->in;
  for (int l = 0; l < nh; ++l) d->width[l + 1] = hid[l];
  d->width[nh + 1] = d->O;
  d->P = dyn_layout(d);
  printf("dyn od=%d ad=%d K=%d floats=%ld config_floats=%lld\n", od, ad, K, d->P, (long long)orl_dyn_config_floats(&c));
  for (int i = 0; i < orl_dyn_num_tensors(d); ++i) {
    char name[160]; int64_t off, sh[4]; int32_t nd;
    if (orl_dyn_tensor(d, i, name, sizeof(name), &off, &nd, sh)) { printf("query failed\n"); return; }
    print_row("dyn", i, name, off, nd, sh);
  }
  delete d;
}

static void diff_case(int od, int ad, int dsed, int nlev, const int* dims, int groups) {
  orl_diffusion_config c;
  orl_diffusion_config_default(&c);
  c.obs_dim = od; c.act_dim = ad; c.step_embed_dim = dsed; c.n_levels = nlev; c.n_groups = groups;
  for (int i = 0; i < nlev; ++i) c.down_dims[i] = dims[i];
  orl_diffusion* d = new orl_diffusion();
  d->c = c;
  d->od = od; d->ad = ad; d->dsed = dsed; d->cond = dsed + od; d->N = c.num_diffusion_iters; d->B = c.batch_size; d->G = groups; d->nlev = nlev;
  d->P = diff_layout(d);
  printf("diffusion od=%d ad=%d levels=%d floats=%ld norm_off=%ld norm_n=%ld film_cols=%d\n", od, ad, nlev, d->P, d->norm_off, d->norm_n, d->film_cols);
  for (int i = 0; i < orl_diffusion_num_tensors(d); ++i) {
    char name[160]; int64_t off, sh[4]; int32_t nd;
    if (orl_diffusion_tensor(d, i, name, sizeof(name), &off, &nd, sh)) { printf("query failed\n"); return; }
    print_row("diffusion", i, name, off, nd, sh);
  }
  // a query past the end must fail, and a short name buffer must stay terminated
  char tiny[5]; int64_t off, sh[4]; int32_t nd;
  printf("past-the-end rc=%d  short-name rc=%d '%s'\n", orl_diffusion_tensor(d, orl_diffusion_num_tensors(d), tiny, 5, &off, &nd, sh),
         orl_diffusion_tensor(d, 0, tiny, 5, &off, &nd, sh), tiny);
  delete d;
}

int main() {
  const int h1[2] = {10, 7}, h2[4] = {200, 200, 200, 200};
  dyn_case(5, 2, 2, h1, 3, 1);
  dyn_case(17, 6, 4, h2, 7, 1);
  const int d1[3] = {8, 16, 32}, d2[3] = {256, 512, 1024};
  diff_case(5, 3, 16, 3, d1, 8);
  diff_case(11, 3, 256, 3, d2, 8);
  return 0;
}
