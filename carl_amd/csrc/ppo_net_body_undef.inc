// ppo_net_body_undef.inc -- takes back the macros a kernel defined for ppo_net_body.inc
#undef PPO_MB_LANE_WINDOW
#undef PPO_MB_LANE_LO
#undef PPO_MB_LANE_HI
#undef PPO_MB_PARAMS
#undef PPO_MB_XFORM
#undef PPO_MB_LOG_STD
#undef PPO_MB_SLAB
#undef PPO_MB_NEW_OUT
#undef PPO_MB_IDX
#undef PPO_MB_ADV_NORM
#undef PPO_MB_CLIP_RANGE
#undef PPO_MB_VF_COEF
#undef PPO_MB_ENT_COEF
