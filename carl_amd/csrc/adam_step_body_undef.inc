// adam_step_body_undef.inc -- takes back the macros a kernel defined for adam_step_body.inc
#undef ADAM_MB_ROW
#undef ADAM_MB_STEP
#undef ADAM_MB_BETA_POW
#undef ADAM_MB_NORM_OUT
#undef ADAM_MB_LR
#undef ADAM_MB_MAX_GRAD_NORM
