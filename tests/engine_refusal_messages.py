"""The outcomes test_engine_refusals.py expects, as literals: (exception type, full message) -- ("Launched", the library
function) where every check passed.  TENSORS maps each spoiled argument's outcomes to the spoils that end in them.
Written by ``python tests/test_engine_refusals.py``; review the diff of a regeneration like any other."""

LAUNCHES = {'gae': ('Launched', 'carl_gae'),
 'context_trace': ('Launched', 'carl_policy_context_trace'),
 'context_trace/brax': ('Launched', 'carl_brax_policy_context_trace'),
 'ppo_grad': ('Launched', 'carl_ppo_grad'),
 'ppo_grad/pendulum': ('Launched', 'carl_ppo_grad'),
 'ppo_grad/brax': ('Launched', 'carl_brax_ppo_grad'),
 'ppo_grad_sets': ('Launched', 'carl_ppo_grad_sets'),
 'ppo_input_stats': ('Launched', 'carl_ppo_input_stats'),
 'ppo_input_stats/brax': ('Launched', 'carl_brax_ppo_input_stats'),
 'ppo_return_stats': ('Launched', 'carl_ppo_return_stats'),
 'ppo_return_merge': ('Launched', 'carl_ppo_return_merge'),
 'ppo_adv_stats': ('Launched', 'carl_ppo_adv_stats'),
 'ppo_adv_stats/flat': ('Launched', 'carl_ppo_adv_stats'),
 'ppo_adv_stats_sets': ('Launched', 'carl_ppo_adv_stats_sets'),
 'ppo_adv_stats_sets/flat': ('Launched', 'carl_ppo_adv_stats_sets'),
 'adam_step': ('Launched', 'carl_adam_step'),
 'adam_step_sets': ('Launched', 'carl_adam_step_sets'),
 'rollout_policy': ('Launched', 'carl_rollout_policy_valued'),
 'rollout_policy/pendulum': ('Launched', 'carl_rollout_policy_valued'),
 'rollout_policy/brax': ('Launched', 'carl_brax_rollout_policy_valued'),
 'rollout_policy/summary': ('Launched', 'carl_rollout_policy'),
 'rollout_policy/brax/summary': ('Launched', 'carl_brax_rollout_policy'),
 'evaluate_policy': ('Launched', 'carl_evaluate_policy_stats'),
 'evaluate_episodes': ('Launched', 'carl_brax_evaluate_policy_stats'),
 'InputStats.update': ('Launched', 'carl_policy_stats_merge')}

TENSORS = {'gae': {'reward': {('ValueError', "gae 'reward': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float64 (3, 24) strides (32, 1)"): 'dtype',
                    ('ValueError', "gae 'reward': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'device',
                    ('ValueError', 'too many values to unpack (expected 2)'): 'rank',
                    ('ValueError', "gae 'value': needs torch.float32 [3, 25] rows of pitch 25 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'last_dim',
                    ('ValueError', "gae 'reward': needs torch.float32 [3, 24] rows of pitch 48 on cpu, got torch.float32 (3, 24) strides (48, 2)"): 'last_strided',
                    ('ValueError', "gae 'value': needs torch.float32 [2, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'fewer_rows',
                    ('ValueError', "gae 'value': needs torch.float32 [4, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'more_rows',
                    ('ValueError', "gae 'value': needs torch.float32 [3, 25] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'lanes',
                    ('ValueError', "gae 'reward': needs torch.float32 [3, 24] rows of pitch 64 on cpu, got torch.float32 (3, 24) strides (64, 2)"): 'lane_strided',
                    ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 24 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'pitch',
                    ('ValueError', "gae 'reward': rows of pitch 0 < 24 lanes"): 'pitch_zero'},
         'value': {('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float64 (3, 24) strides (32, 1)"): 'dtype',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'device',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (1, 3, 24) strides (96, 32, 1)"): 'rank',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (25, 1)"): 'last_dim',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (48, 2)"): 'last_strided',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (2, 24) strides (32, 1)"): 'fewer_rows',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (4, 24) strides (32, 1)"): 'more_rows',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (32, 1)"): 'lanes',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (64, 2)"): 'lane_strided',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (24, 1)"): 'pitch',
                   ('ValueError', "gae 'value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (0, 1)"): 'pitch_zero'},
         'terminated': {('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.float64 (3, 24) strides (32, 1)"): 'dtype',
                        ('Launched', 'carl_gae'): 'bool',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (32, 1)"): 'device',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (1, 3, 24) strides (96, 32, 1)"): 'rank',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 25) strides (25, 1)"): 'last_dim',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (48, 2)"): 'last_strided',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (2, 24) strides (32, 1)"): 'fewer_rows',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (4, 24) strides (32, 1)"): 'more_rows',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 25) strides (32, 1)"): 'lanes',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (64, 2)"): 'lane_strided',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (24, 1)"): 'pitch',
                        ('ValueError', "gae 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (0, 1)"): 'pitch_zero'},
         'truncated': {('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.float64 (3, 24) strides (32, 1)"): 'dtype',
                       ('Launched', 'carl_gae'): 'bool',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (32, 1)"): 'device',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (1, 3, 24) strides (96, 32, 1)"): 'rank',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 25) strides (25, 1)"): 'last_dim',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (48, 2)"): 'last_strided',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (2, 24) strides (32, 1)"): 'fewer_rows',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (4, 24) strides (32, 1)"): 'more_rows',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 25) strides (32, 1)"): 'lanes',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (64, 2)"): 'lane_strided',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (24, 1)"): 'pitch',
                       ('ValueError', "gae 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu, got torch.uint8 (3, 24) strides (0, 1)"): 'pitch_zero'},
         'last_value': {('ValueError', "gae 'last_value': needs a contiguous float32 [24] tensor on cpu"): 'device dtype fewer_rows last_dim '
                                                                                                           'last_strided rank'},
         'boot_value': {('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float64 (3, 24) strides (32, 1)"): 'dtype',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'device',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (1, 3, 24) strides (96, 32, 1)"): 'rank',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (25, 1)"): 'last_dim',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (48, 2)"): 'last_strided',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (2, 24) strides (32, 1)"): 'fewer_rows',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (4, 24) strides (32, 1)"): 'more_rows',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (32, 1)"): 'lanes',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (64, 2)"): 'lane_strided',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (24, 1)"): 'pitch',
                        ('ValueError', "gae 'boot_value': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (0, 1)"): 'pitch_zero'},
         'out.advantage': {('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float64 (3, 24) strides (32, 1)"): 'dtype',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'device',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (1, 3, 24) strides (96, 32, 1)"): 'rank',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (25, 1)"): 'last_dim',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (48, 2)"): 'last_strided',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (2, 24) strides (32, 1)"): 'fewer_rows',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (4, 24) strides (32, 1)"): 'more_rows',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (32, 1)"): 'lanes',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (64, 2)"): 'lane_strided',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (24, 1)"): 'pitch',
                           ('ValueError', "gae 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (0, 1)"): 'pitch_zero',
                           ('Launched', 'carl_gae'): 'missing'},
         'out.return': {('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float64 (3, 24) strides (32, 1)"): 'dtype',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (32, 1)"): 'device',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (1, 3, 24) strides (96, 32, 1)"): 'rank',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (25, 1)"): 'last_dim',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (48, 2)"): 'last_strided',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (2, 24) strides (32, 1)"): 'fewer_rows',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (4, 24) strides (32, 1)"): 'more_rows',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 25) strides (32, 1)"): 'lanes',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (64, 2)"): 'lane_strided',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (24, 1)"): 'pitch',
                        ('ValueError', "gae 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu, got torch.float32 (3, 24) strides (0, 1)"): 'pitch_zero',
                        ('Launched', 'carl_gae'): 'missing'}},
 'context_trace': {'ctx_idx0': {('ValueError', "context_trace 'ctx_idx0': needs a contiguous int32 [24] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                         'last_dim last_strided '
                                                                                                                         'rank'},
                   'episode0': {('ValueError', "context_trace 'episode0': needs a contiguous int32 [24] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                         'last_dim last_strided '
                                                                                                                         'rank'},
                   'terminated': {('ValueError', "context_trace 'terminated': needs uint8 [3, 24] rows of pitch 32 on cpu"): 'device dtype',
                                  ('Launched', 'carl_policy_context_trace'): 'bool',
                                  ('ValueError', 'too many values to unpack (expected 2)'): 'rank',
                                  ('ValueError', 'context_trace: flag rows of 25 lanes (pitch 25) for an engine of 24'): 'last_dim',
                                  ('ValueError', "context_trace 'terminated': needs uint8 [3, 24] rows of pitch 48 on cpu"): 'last_strided',
                                  ('ValueError', "context_trace 'truncated': needs uint8 [2, 24] rows of pitch 32 on cpu"): 'fewer_rows',
                                  ('ValueError', "context_trace 'truncated': needs uint8 [4, 24] rows of pitch 32 on cpu"): 'more_rows',
                                  ('ValueError', 'context_trace: flag rows of 25 lanes (pitch 32) for an engine of 24'): 'lanes',
                                  ('ValueError', "context_trace 'terminated': needs uint8 [3, 24] rows of pitch 64 on cpu"): 'lane_strided',
                                  ('ValueError', "context_trace 'truncated': needs uint8 [3, 24] rows of pitch 24 on cpu"): 'pitch',
                                  ('ValueError', 'context_trace: flag rows of 24 lanes (pitch 0) for an engine of 24'): 'pitch_zero'},
                   'truncated': {('ValueError', "context_trace 'truncated': needs uint8 [3, 24] rows of pitch 32 on cpu"): 'device dtype fewer_rows '
                                                                                                                           'lane_strided lanes '
                                                                                                                           'last_dim last_strided '
                                                                                                                           'more_rows pitch '
                                                                                                                           'pitch_zero rank',
                                 ('Launched', 'carl_policy_context_trace'): 'bool'},
                   'out': {('ValueError', "context_trace 'out': needs int32 [3, 24] rows of pitch 32 on cpu"): 'device dtype fewer_rows lane_strided '
                                                                                                               'lanes last_dim last_strided '
                                                                                                               'more_rows pitch pitch_zero rank'}},
 'context_trace/brax': {'ctx_idx0': {('ValueError', "context_trace 'ctx_idx0': needs a contiguous int32 [8] tensor on cpu"): 'device dtype '
                                                                                                                             'fewer_rows last_dim '
                                                                                                                             'last_strided rank'},
                        'episode0': {('ValueError', "context_trace 'episode0': needs a contiguous int32 [8] tensor on cpu"): 'device dtype '
                                                                                                                             'fewer_rows last_dim '
                                                                                                                             'last_strided rank'},
                        'terminated': {('ValueError', "context_trace 'terminated': needs uint8 [3, 8] rows of pitch 8 on cpu"): 'device dtype',
                                       ('Launched', 'carl_brax_policy_context_trace'): 'bool',
                                       ('ValueError', 'too many values to unpack (expected 2)'): 'rank',
                                       ('ValueError', 'context_trace: flag rows of 9 lanes (pitch 9) for an engine of 8'): 'lanes last_dim',
                                       ('ValueError', "context_trace 'terminated': needs uint8 [3, 8] rows of pitch 16 on cpu"): 'lane_strided '
                                                                                                                                 'last_strided',
                                       ('ValueError', "context_trace 'truncated': needs uint8 [2, 8] rows of pitch 8 on cpu"): 'fewer_rows',
                                       ('ValueError', "context_trace 'truncated': needs uint8 [4, 8] rows of pitch 8 on cpu"): 'more_rows',
                                       ('ValueError', "context_trace 'truncated': needs uint8 [3, 8] rows of pitch 24 on cpu"): 'pitch',
                                       ('ValueError', 'context_trace: flag rows of 8 lanes (pitch 0) for an engine of 8'): 'pitch_zero'},
                        'truncated': {('ValueError', "context_trace 'truncated': needs uint8 [3, 8] rows of pitch 8 on cpu"): 'device dtype '
                                                                                                                              'fewer_rows '
                                                                                                                              'lane_strided lanes '
                                                                                                                              'last_dim last_strided '
                                                                                                                              'more_rows pitch '
                                                                                                                              'pitch_zero rank',
                                      ('Launched', 'carl_brax_policy_context_trace'): 'bool'},
                        'out': {('ValueError', "context_trace 'out': needs int32 [3, 8] rows of pitch 8 on cpu"): 'device dtype fewer_rows '
                                                                                                                  'lane_strided lanes last_dim '
                                                                                                                  'last_strided more_rows pitch '
                                                                                                                  'pitch_zero rank'}},
 'ppo_grad': {'buf.obs': {('ValueError', "ppo_grad 'obs': needs float32 [3, 24, 4] rows of pitch 32 on cpu"): 'device dtype fewer_rows lane_strided '
                                                                                                              'lanes last_dim last_strided pitch '
                                                                                                              'pitch_zero rank',
                          ('Launched', 'carl_ppo_grad'): 'more_rows',
                          ('KeyError', "'obs'"): 'missing'},
              'buf.action': {('ValueError', "ppo_grad 'action': needs torch.int32 [3, 24] rows of pitch 32 on cpu"): 'device dtype',
                             ('ValueError', 'too many values to unpack (expected 2)'): 'rank',
                             ('ValueError', 'ppo_grad: a buffer of 25 lanes for an engine of 24'): 'lanes last_dim',
                             ('ValueError', "ppo_grad 'action': needs torch.int32 [3, 24] rows of pitch 48 on cpu"): 'last_strided',
                             ('Launched', 'carl_ppo_grad'): 'fewer_rows',
                             ('ValueError', "ppo_grad 'log_prob': needs torch.float32 [4, 24] rows of pitch 32 on cpu"): 'more_rows',
                             ('ValueError', "ppo_grad 'action': needs torch.int32 [3, 24] rows of pitch 64 on cpu"): 'lane_strided',
                             ('ValueError', "ppo_grad 'log_prob': needs torch.float32 [3, 24] rows of pitch 24 on cpu"): 'pitch',
                             ('ValueError', "ppo_grad 'log_prob': needs torch.float32 [3, 24] rows of pitch 0 on cpu"): 'pitch_zero',
                             ('KeyError', "'action'"): 'missing'},
              'buf.log_prob': {('ValueError', "ppo_grad 'log_prob': needs torch.float32 [3, 24] rows of pitch 32 on cpu"): 'device dtype fewer_rows '
                                                                                                                           'lane_strided lanes '
                                                                                                                           'last_dim last_strided '
                                                                                                                           'pitch pitch_zero rank',
                               ('Launched', 'carl_ppo_grad'): 'more_rows',
                               ('KeyError', "'log_prob'"): 'missing'},
              'buf.advantage': {('ValueError', "ppo_grad 'advantage': needs torch.float32 [3, 24] rows of pitch 32 on cpu"): 'device dtype '
                                                                                                                             'fewer_rows '
                                                                                                                             'lane_strided lanes '
                                                                                                                             'last_dim last_strided '
                                                                                                                             'pitch pitch_zero rank',
                                ('Launched', 'carl_ppo_grad'): 'more_rows',
                                ('KeyError', "'advantage'"): 'missing'},
              'buf.return': {('ValueError', "ppo_grad 'return': needs torch.float32 [3, 24] rows of pitch 32 on cpu"): 'device dtype fewer_rows '
                                                                                                                       'lane_strided lanes last_dim '
                                                                                                                       'last_strided pitch '
                                                                                                                       'pitch_zero rank',
                             ('Launched', 'carl_ppo_grad'): 'more_rows',
                             ('KeyError', "'return'"): 'missing'},
              'obs0': {('ValueError', "ppo_grad 'obs0': needs a contiguous float32 [24, 4] tensor on cpu"): 'device dtype fewer_rows lane_strided '
                                                                                                            'lanes last_dim last_strided more_rows '
                                                                                                            'pitch pitch_zero rank'},
              'context_id': {('ValueError', "ppo_grad 'context_id': needs torch.int32 [3, 24] rows of pitch 32 on cpu"): 'device dtype fewer_rows '
                                                                                                                         'lane_strided lanes '
                                                                                                                         'last_dim last_strided '
                                                                                                                         'pitch pitch_zero rank',
                             ('Launched', 'carl_ppo_grad'): 'more_rows'},
              'idx': {('ValueError', "ppo_grad 'idx': needs a contiguous int32 [M] tensor on cpu"): 'device dtype last_strided rank',
                      ('ValueError', "ppo_grad output 'new_log_prob': needs a contiguous float32 [6] tensor on cpu"): 'last_dim',
                      ('ValueError', "ppo_grad output 'new_log_prob': needs a contiguous float32 [4] tensor on cpu"): 'fewer_rows'},
              'adv_norm': {('ValueError', "ppo_grad 'adv_norm': needs a contiguous float32 [2] tensor on cpu"): 'device dtype fewer_rows last_dim '
                                                                                                                'last_strided',
                           ('Launched', 'carl_ppo_grad'): 'rank'},
              'out.grad_actor': {('ValueError', "ppo_grad output 'grad_actor': needs a contiguous float32 [148] tensor on cpu"): 'device dtype '
                                                                                                                                 'fewer_rows '
                                                                                                                                 'last_dim '
                                                                                                                                 'last_strided',
                                 ('Launched', 'carl_ppo_grad'): 'missing rank'},
              'out.grad_critic': {('ValueError', "ppo_grad output 'grad_critic': needs a contiguous float32 [140] tensor on cpu"): 'device dtype '
                                                                                                                                   'fewer_rows '
                                                                                                                                   'last_dim '
                                                                                                                                   'last_strided',
                                  ('Launched', 'carl_ppo_grad'): 'missing rank'},
              'out.stats': {('ValueError', "ppo_grad output 'stats': needs a contiguous float32 [6] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                     'last_dim last_strided',
                            ('Launched', 'carl_ppo_grad'): 'missing rank'},
              'out.new_log_prob': {('ValueError', "ppo_grad output 'new_log_prob': needs a contiguous float32 [5] tensor on cpu"): 'device dtype '
                                                                                                                                   'fewer_rows '
                                                                                                                                   'last_dim '
                                                                                                                                   'last_strided',
                                   ('Launched', 'carl_ppo_grad'): 'missing rank'},
              'out.new_value': {('ValueError', "ppo_grad output 'new_value': needs a contiguous float32 [5] tensor on cpu"): 'device dtype '
                                                                                                                             'fewer_rows last_dim '
                                                                                                                             'last_strided',
                                ('Launched', 'carl_ppo_grad'): 'missing rank'}},
 'ppo_grad/pendulum': {'buf.action': {('ValueError', "ppo_grad 'action': needs torch.float32 [3, 24] rows of pitch 32 on cpu"): 'device dtype',
                                      ('ValueError', 'too many values to unpack (expected 2)'): 'rank',
                                      ('ValueError', 'ppo_grad: a buffer of 25 lanes for an engine of 24'): 'lanes last_dim',
                                      ('ValueError', "ppo_grad 'action': needs torch.float32 [3, 24] rows of pitch 48 on cpu"): 'last_strided',
                                      ('Launched', 'carl_ppo_grad'): 'fewer_rows',
                                      ('ValueError', "ppo_grad 'log_prob': needs torch.float32 [4, 24] rows of pitch 32 on cpu"): 'more_rows',
                                      ('ValueError', "ppo_grad 'action': needs torch.float32 [3, 24] rows of pitch 64 on cpu"): 'lane_strided',
                                      ('ValueError', "ppo_grad 'log_prob': needs torch.float32 [3, 24] rows of pitch 24 on cpu"): 'pitch',
                                      ('ValueError', "ppo_grad 'log_prob': needs torch.float32 [3, 24] rows of pitch 0 on cpu"): 'pitch_zero',
                                      ('KeyError', "'action'"): 'missing'},
                       'out.grad_log_std': {('ValueError', "ppo_grad output 'grad_log_std': needs a contiguous float32 [1] tensor on cpu"): 'device '
                                                                                                                                            'dtype '
                                                                                                                                            'last_dim',
                                            ('Launched', 'carl_ppo_grad'): 'last_strided missing rank'}},
 'ppo_grad/brax': {'buf.obs': {('ValueError', "ppo_grad 'obs': needs float32 [3, 8, 27] rows of pitch 8 on cpu"): 'device dtype fewer_rows '
                                                                                                                  'lane_strided lanes last_dim '
                                                                                                                  'last_strided pitch pitch_zero '
                                                                                                                  'rank',
                               ('Launched', 'carl_brax_ppo_grad'): 'more_rows',
                               ('KeyError', "'obs'"): 'missing'},
                   'buf.action': {('ValueError', "ppo_grad 'action': needs a contiguous float32 [T, 8, 8] tensor on cpu"): 'device dtype '
                                                                                                                           'lane_strided last_dim '
                                                                                                                           'last_strided pitch '
                                                                                                                           'pitch_zero rank',
                                  ('Launched', 'carl_brax_ppo_grad'): 'fewer_rows',
                                  ('ValueError', "ppo_grad 'log_prob': needs torch.float32 [4, 8] rows of pitch 8 on cpu"): 'more_rows',
                                  ('ValueError', 'ppo_grad: a buffer of 9 lanes for an engine of 8'): 'lanes',
                                  ('KeyError', "'action'"): 'missing'},
                   'buf.log_prob': {('ValueError', "ppo_grad 'log_prob': needs torch.float32 [3, 8] rows of pitch 8 on cpu"): 'device dtype '
                                                                                                                              'fewer_rows '
                                                                                                                              'lane_strided lanes '
                                                                                                                              'last_dim last_strided '
                                                                                                                              'pitch pitch_zero rank',
                                    ('Launched', 'carl_brax_ppo_grad'): 'more_rows',
                                    ('KeyError', "'log_prob'"): 'missing'},
                   'buf.advantage': {('ValueError', "ppo_grad 'advantage': needs torch.float32 [3, 8] rows of pitch 8 on cpu"): 'device dtype '
                                                                                                                                'fewer_rows '
                                                                                                                                'lane_strided lanes '
                                                                                                                                'last_dim '
                                                                                                                                'last_strided pitch '
                                                                                                                                'pitch_zero rank',
                                     ('Launched', 'carl_brax_ppo_grad'): 'more_rows',
                                     ('KeyError', "'advantage'"): 'missing'},
                   'buf.return': {('ValueError', "ppo_grad 'return': needs torch.float32 [3, 8] rows of pitch 8 on cpu"): 'device dtype fewer_rows '
                                                                                                                          'lane_strided lanes '
                                                                                                                          'last_dim last_strided '
                                                                                                                          'pitch pitch_zero rank',
                                  ('Launched', 'carl_brax_ppo_grad'): 'more_rows',
                                  ('KeyError', "'return'"): 'missing'},
                   'obs0': {('ValueError', "ppo_grad 'obs0': needs a contiguous float32 [8, 27] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                 'lane_strided lanes last_dim '
                                                                                                                 'last_strided more_rows pitch '
                                                                                                                 'pitch_zero rank'},
                   'context_id': {('ValueError', "ppo_grad 'context_id': needs torch.int32 [3, 8] rows of pitch 8 on cpu"): 'device dtype fewer_rows '
                                                                                                                            'lane_strided lanes '
                                                                                                                            'last_dim last_strided '
                                                                                                                            'pitch pitch_zero rank',
                                  ('Launched', 'carl_brax_ppo_grad'): 'more_rows'},
                   'idx': {('ValueError', "ppo_grad 'idx': needs a contiguous int32 [M] tensor on cpu"): 'device dtype last_strided rank',
                           ('ValueError', "ppo_grad output 'new_log_prob': needs a contiguous float32 [6] tensor on cpu"): 'last_dim',
                           ('ValueError', "ppo_grad output 'new_log_prob': needs a contiguous float32 [4] tensor on cpu"): 'fewer_rows'},
                   'adv_norm': {('ValueError', "ppo_grad 'adv_norm': needs a contiguous float32 [2] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                     'last_dim last_strided',
                                ('Launched', 'carl_brax_ppo_grad'): 'rank'},
                   'out.grad_actor': {('ValueError', "ppo_grad output 'grad_actor': needs a contiguous float32 [352] tensor on cpu"): 'device dtype '
                                                                                                                                      'fewer_rows '
                                                                                                                                      'last_dim '
                                                                                                                                      'last_strided',
                                      ('Launched', 'carl_brax_ppo_grad'): 'missing rank'},
                   'out.grad_critic': {('ValueError', "ppo_grad output 'grad_critic': needs a contiguous float32 [288] tensor on cpu"): 'device '
                                                                                                                                        'dtype '
                                                                                                                                        'fewer_rows '
                                                                                                                                        'last_dim '
                                                                                                                                        'last_strided',
                                       ('Launched', 'carl_brax_ppo_grad'): 'missing rank'},
                   'out.stats': {('ValueError', "ppo_grad output 'stats': needs a contiguous float32 [6] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                          'last_dim last_strided',
                                 ('Launched', 'carl_brax_ppo_grad'): 'missing rank'},
                   'out.new_log_prob': {('ValueError', "ppo_grad output 'new_log_prob': needs a contiguous float32 [5] tensor on cpu"): 'device '
                                                                                                                                        'dtype '
                                                                                                                                        'fewer_rows '
                                                                                                                                        'last_dim '
                                                                                                                                        'last_strided',
                                        ('Launched', 'carl_brax_ppo_grad'): 'missing rank'},
                   'out.new_value': {('ValueError', "ppo_grad output 'new_value': needs a contiguous float32 [5] tensor on cpu"): 'device dtype '
                                                                                                                                  'fewer_rows '
                                                                                                                                  'last_dim '
                                                                                                                                  'last_strided',
                                     ('Launched', 'carl_brax_ppo_grad'): 'missing rank'},
                   'out.grad_log_std': {('ValueError', "ppo_grad output 'grad_log_std': needs a contiguous float32 [8] tensor on cpu"): 'device '
                                                                                                                                        'dtype '
                                                                                                                                        'fewer_rows '
                                                                                                                                        'last_dim '
                                                                                                                                        'last_strided',
                                        ('Launched', 'carl_brax_ppo_grad'): 'missing rank'}},
 'ppo_grad_sets': {'buf.obs': {('ValueError', "ppo_grad_sets 'obs': needs float32 [3, 512, 4] rows of pitch 512 on cpu"): 'device dtype fewer_rows '
                                                                                                                          'lane_strided lanes '
                                                                                                                          'last_dim last_strided '
                                                                                                                          'pitch pitch_zero rank',
                               ('Launched', 'carl_ppo_grad_sets'): 'more_rows',
                               ('KeyError', "'obs'"): 'missing'},
                   'buf.action': {('ValueError', "ppo_grad_sets 'action': needs torch.int32 [3, 512] rows of pitch 512 on cpu"): 'device dtype',
                                  ('ValueError', 'too many values to unpack (expected 2)'): 'rank',
                                  ('ValueError', 'ppo_grad_sets: a buffer of 513 lanes for an engine of 512'): 'lanes last_dim',
                                  ('ValueError', "ppo_grad_sets 'action': needs torch.int32 [3, 512] rows of pitch 1024 on cpu"): 'lane_strided '
                                                                                                                                  'last_strided',
                                  ('Launched', 'carl_ppo_grad_sets'): 'fewer_rows',
                                  ('ValueError', "ppo_grad_sets 'log_prob': needs torch.float32 [4, 512] rows of pitch 512 on cpu"): 'more_rows',
                                  ('ValueError', "ppo_grad_sets 'log_prob': needs torch.float32 [3, 512] rows of pitch 528 on cpu"): 'pitch',
                                  ('ValueError', "ppo_grad_sets 'log_prob': needs torch.float32 [3, 512] rows of pitch 0 on cpu"): 'pitch_zero',
                                  ('KeyError', "'action'"): 'missing'},
                   'obs0': {('ValueError', "ppo_grad_sets 'obs0': needs a contiguous float32 [512, 4] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                       'lane_strided lanes last_dim '
                                                                                                                       'last_strided more_rows pitch '
                                                                                                                       'pitch_zero rank'},
                   'context_id': {('ValueError', "ppo_grad_sets 'context_id': needs torch.int32 [3, 512] rows of pitch 512 on cpu"): 'device dtype '
                                                                                                                                     'fewer_rows '
                                                                                                                                     'lane_strided '
                                                                                                                                     'lanes last_dim '
                                                                                                                                     'last_strided '
                                                                                                                                     'pitch '
                                                                                                                                     'pitch_zero '
                                                                                                                                     'rank',
                                  ('Launched', 'carl_ppo_grad_sets'): 'more_rows'},
                   'idx': {('ValueError', "ppo_grad_sets 'idx': needs int32 [2, M >= 1] rows of unit stride on cpu"): 'device dtype fewer_rows '
                                                                                                                      'lane_strided last_strided '
                                                                                                                      'more_rows pitch_zero rank',
                           ('Launched', 'carl_ppo_grad_sets'): 'lanes last_dim pitch'},
                   'hyper': {('ValueError', "ppo_grad_sets 'hyper': needs a contiguous float64 [2, 5] tensor on cpu (columns lr, clip_range, vf_coef, ent_coef, max_grad_norm)"): 'device '
                                                                                                                                                                                  'dtype '
                                                                                                                                                                                  'fewer_rows '
                                                                                                                                                                                  'lane_strided '
                                                                                                                                                                                  'lanes '
                                                                                                                                                                                  'last_dim '
                                                                                                                                                                                  'last_strided '
                                                                                                                                                                                  'more_rows '
                                                                                                                                                                                  'pitch '
                                                                                                                                                                                  'pitch_zero '
                                                                                                                                                                                  'rank'},
                   'adv_norm': {('ValueError', "ppo_grad_sets 'adv_norm': needs float32 [2, 2] rows of unit stride on cpu"): 'device dtype '
                                                                                                                             'fewer_rows '
                                                                                                                             'lane_strided lanes '
                                                                                                                             'last_dim last_strided '
                                                                                                                             'more_rows pitch_zero '
                                                                                                                             'rank',
                                ('Launched', 'carl_ppo_grad_sets'): 'pitch'},
                   'out.grad_actor': {('ValueError', "ppo_grad_sets output 'grad_actor': needs a contiguous float32 [2, 148] tensor on cpu"): 'device '
                                                                                                                                              'dtype '
                                                                                                                                              'fewer_rows '
                                                                                                                                              'lane_strided '
                                                                                                                                              'lanes '
                                                                                                                                              'last_dim '
                                                                                                                                              'last_strided '
                                                                                                                                              'more_rows '
                                                                                                                                              'pitch '
                                                                                                                                              'pitch_zero '
                                                                                                                                              'rank',
                                      ('Launched', 'carl_ppo_grad_sets'): 'missing'},
                   'out.grad_critic': {('ValueError', "ppo_grad_sets output 'grad_critic': needs a contiguous float32 [2, 140] tensor on cpu"): 'device '
                                                                                                                                                'dtype '
                                                                                                                                                'fewer_rows '
                                                                                                                                                'lane_strided '
                                                                                                                                                'lanes '
                                                                                                                                                'last_dim '
                                                                                                                                                'last_strided '
                                                                                                                                                'more_rows '
                                                                                                                                                'pitch '
                                                                                                                                                'pitch_zero '
                                                                                                                                                'rank',
                                       ('Launched', 'carl_ppo_grad_sets'): 'missing'},
                   'out.stats': {('ValueError', "ppo_grad_sets output 'stats': needs a contiguous float32 [2, 6] tensor on cpu"): 'device dtype '
                                                                                                                                  'fewer_rows '
                                                                                                                                  'lane_strided '
                                                                                                                                  'lanes last_dim '
                                                                                                                                  'last_strided '
                                                                                                                                  'more_rows pitch '
                                                                                                                                  'pitch_zero rank',
                                 ('Launched', 'carl_ppo_grad_sets'): 'missing'}},
 'ppo_input_stats': {'buf.obs': {('ValueError', "ppo_input_stats 'obs': needs float32 [3, 24, 4] rows of pitch 32 on cpu"): 'device dtype fewer_rows '
                                                                                                                            'lane_strided lanes '
                                                                                                                            'last_dim last_strided '
                                                                                                                            'pitch pitch_zero rank',
                                 ('Launched', 'carl_ppo_input_stats'): 'more_rows',
                                 ('KeyError', "'obs'"): 'missing'},
                     'obs0': {('ValueError', "ppo_input_stats 'obs0': needs a contiguous float32 [24, 4] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                          'lane_strided lanes '
                                                                                                                          'last_dim last_strided '
                                                                                                                          'more_rows pitch '
                                                                                                                          'pitch_zero rank'},
                     'context_id': {('ValueError', "ppo_input_stats 'context_id': needs int32 [3, 24] rows of pitch 32 on cpu"): 'device dtype',
                                    ('ValueError', "ppo_input_stats 'context_id': needs int32 [T, 24] rows on cpu"): 'rank',
                                    ('ValueError', 'ppo_input_stats: a buffer of 3 steps x 25 lanes for an engine of 24'): 'lanes last_dim',
                                    ('ValueError', "ppo_input_stats 'context_id': needs int32 [3, 24] rows of pitch 48 on cpu"): 'last_strided',
                                    ('Launched', 'carl_ppo_input_stats'): 'fewer_rows',
                                    ('ValueError', "ppo_input_stats 'obs': needs float32 [4, 24, 4] rows of pitch 32 on cpu"): 'more_rows',
                                    ('ValueError', "ppo_input_stats 'context_id': needs int32 [3, 24] rows of pitch 64 on cpu"): 'lane_strided',
                                    ('ValueError', "ppo_input_stats 'obs': needs float32 [3, 24, 4] rows of pitch 24 on cpu"): 'pitch',
                                    ('ValueError', "ppo_input_stats 'context_id': needs int32 [3, 24] rows of pitch 0 on cpu"): 'pitch_zero'},
                     'out.input_partial': {('ValueError', "ppo_input_stats 'input_partial': needs a contiguous float64 [>= 1, 2, 32] tensor on cpu"): 'device '
                                                                                                                                                      'dtype '
                                                                                                                                                      'lane_strided '
                                                                                                                                                      'lanes '
                                                                                                                                                      'last_dim '
                                                                                                                                                      'last_strided '
                                                                                                                                                      'rank',
                                           ('Launched', 'carl_ppo_input_stats'): 'missing more_rows pitch pitch_zero'},
                     'out.steps': {('ValueError', "ppo_input_stats 'steps': needs a contiguous int32 [24] tensor on cpu (filled with T)"): 'device '
                                                                                                                                           'dtype '
                                                                                                                                           'fewer_rows '
                                                                                                                                           'last_dim '
                                                                                                                                           'last_strided '
                                                                                                                                           'rank',
                                   ('Launched', 'carl_ppo_input_stats'): 'missing'}},
 'ppo_input_stats/brax': {'buf.obs': {('ValueError', "ppo_input_stats 'obs': needs float32 [3, 8, 27] rows of pitch 8 on cpu"): 'device dtype '
                                                                                                                                'fewer_rows '
                                                                                                                                'lane_strided lanes '
                                                                                                                                'last_dim '
                                                                                                                                'last_strided pitch '
                                                                                                                                'pitch_zero rank',
                                      ('Launched', 'carl_brax_ppo_input_stats'): 'more_rows',
                                      ('KeyError', "'obs'"): 'missing'},
                          'obs0': {('ValueError', "ppo_input_stats 'obs0': needs a contiguous float32 [8, 27] tensor on cpu"): 'device dtype '
                                                                                                                               'fewer_rows '
                                                                                                                               'lane_strided lanes '
                                                                                                                               'last_dim '
                                                                                                                               'last_strided '
                                                                                                                               'more_rows pitch '
                                                                                                                               'pitch_zero rank'},
                          'context_id': {('ValueError', "ppo_input_stats 'context_id': needs int32 [3, 8] rows of pitch 8 on cpu"): 'device dtype '
                                                                                                                                    'lane_strided '
                                                                                                                                    'last_strided '
                                                                                                                                    'pitch '
                                                                                                                                    'pitch_zero',
                                         ('ValueError', "ppo_input_stats 'context_id': needs int32 [T, 8] rows on cpu"): 'rank',
                                         ('ValueError', 'ppo_input_stats: a buffer of 3 steps x 9 lanes for an engine of 8'): 'lanes last_dim',
                                         ('Launched', 'carl_brax_ppo_input_stats'): 'fewer_rows',
                                         ('ValueError', "ppo_input_stats 'obs': needs float32 [4, 8, 27] rows of pitch 8 on cpu"): 'more_rows'},
                          'out.input_partial': {('ValueError', "ppo_input_stats 'input_partial': needs a contiguous float64 [>= 1, 2, 32] tensor on cpu"): 'device '
                                                                                                                                                           'dtype '
                                                                                                                                                           'lane_strided '
                                                                                                                                                           'lanes '
                                                                                                                                                           'last_dim '
                                                                                                                                                           'last_strided '
                                                                                                                                                           'rank',
                                                ('Launched', 'carl_brax_ppo_input_stats'): 'missing more_rows pitch pitch_zero'},
                          'out.steps': {('ValueError', "ppo_input_stats 'steps': needs a contiguous int32 [8] tensor on cpu (filled with T)"): 'device '
                                                                                                                                               'dtype '
                                                                                                                                               'fewer_rows '
                                                                                                                                               'last_dim '
                                                                                                                                               'last_strided '
                                                                                                                                               'rank',
                                        ('Launched', 'carl_brax_ppo_input_stats'): 'missing'}},
 'ppo_return_stats': {'reward': {('ValueError', "ppo_return_stats 'reward': needs torch.float32 [3, 24] rows of pitch 32 on cpu"): 'device dtype',
                                 ('ValueError', 'too many values to unpack (expected 2)'): 'rank',
                                 ('ValueError', 'ppo_return_stats: reward rows of 3 steps x 25 lanes (pitch 25) for an engine of 24'): 'last_dim',
                                 ('ValueError', "ppo_return_stats 'reward': needs torch.float32 [3, 24] rows of pitch 48 on cpu"): 'last_strided',
                                 ('ValueError', "ppo_return_stats 'terminated': needs torch.uint8 [2, 24] rows of pitch 32 on cpu"): 'fewer_rows',
                                 ('ValueError', "ppo_return_stats 'terminated': needs torch.uint8 [4, 24] rows of pitch 32 on cpu"): 'more_rows',
                                 ('ValueError', 'ppo_return_stats: reward rows of 3 steps x 25 lanes (pitch 32) for an engine of 24'): 'lanes',
                                 ('ValueError', "ppo_return_stats 'reward': needs torch.float32 [3, 24] rows of pitch 64 on cpu"): 'lane_strided',
                                 ('ValueError', "ppo_return_stats 'terminated': needs torch.uint8 [3, 24] rows of pitch 24 on cpu"): 'pitch',
                                 ('ValueError', 'ppo_return_stats: reward rows of 3 steps x 24 lanes (pitch 0) for an engine of 24'): 'pitch_zero'},
                      'terminated': {('ValueError', "ppo_return_stats 'terminated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu"): 'device '
                                                                                                                                         'dtype '
                                                                                                                                         'fewer_rows '
                                                                                                                                         'lane_strided '
                                                                                                                                         'lanes '
                                                                                                                                         'last_dim '
                                                                                                                                         'last_strided '
                                                                                                                                         'more_rows '
                                                                                                                                         'pitch '
                                                                                                                                         'pitch_zero '
                                                                                                                                         'rank',
                                     ('Launched', 'carl_ppo_return_stats'): 'bool'},
                      'truncated': {('ValueError', "ppo_return_stats 'truncated': needs torch.uint8 [3, 24] rows of pitch 32 on cpu"): 'device dtype '
                                                                                                                                       'fewer_rows '
                                                                                                                                       'lane_strided '
                                                                                                                                       'lanes '
                                                                                                                                       'last_dim '
                                                                                                                                       'last_strided '
                                                                                                                                       'more_rows '
                                                                                                                                       'pitch '
                                                                                                                                       'pitch_zero '
                                                                                                                                       'rank',
                                    ('Launched', 'carl_ppo_return_stats'): 'bool'},
                      'ret': {('ValueError', "ppo_return_stats 'ret': needs a contiguous float32 [24] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                       'last_dim last_strided rank'},
                      'out.return_partial': {('ValueError', "ppo_return_stats 'return_partial': needs a contiguous float64 [1, 2] tensor on cpu"): 'device '
                                                                                                                                                   'dtype '
                                                                                                                                                   'lane_strided '
                                                                                                                                                   'lanes '
                                                                                                                                                   'last_dim '
                                                                                                                                                   'last_strided '
                                                                                                                                                   'more_rows '
                                                                                                                                                   'rank',
                                             ('Launched', 'carl_ppo_return_stats'): 'missing pitch pitch_zero'},
                      'out.ret_rows': {('ValueError', "ppo_return_stats 'ret_rows': needs float32 [3, 24] rows of pitch 32 on cpu"): 'device dtype '
                                                                                                                                     'fewer_rows '
                                                                                                                                     'lane_strided '
                                                                                                                                     'lanes last_dim '
                                                                                                                                     'last_strided '
                                                                                                                                     'more_rows '
                                                                                                                                     'pitch '
                                                                                                                                     'pitch_zero '
                                                                                                                                     'rank',
                                       ('Launched', 'carl_ppo_return_stats'): 'missing'}},
 'ppo_return_merge': {'partial': {('ValueError', "ppo_return_merge 'partial': needs a contiguous float64 [slabs, 2] tensor on cpu"): 'device dtype '
                                                                                                                                     'lane_strided '
                                                                                                                                     'lanes last_dim '
                                                                                                                                     'last_strided '
                                                                                                                                     'pitch '
                                                                                                                                     'pitch_zero '
                                                                                                                                     'rank',
                                  ('Launched', 'carl_ppo_return_merge'): 'fewer_rows more_rows'},
                      'running.count': {('ValueError', "ppo_return_merge running['count']: needs a torch.int64 [1] tensor on cpu"): 'device dtype '
                                                                                                                                    'last_dim',
                                        ('Launched', 'carl_ppo_return_merge'): 'last_strided rank',
                                        ('KeyError', "'count'"): 'missing'},
                      'running.mean': {('ValueError', "ppo_return_merge running['mean']: needs a torch.float64 [1] tensor on cpu"): 'device dtype '
                                                                                                                                    'last_dim',
                                       ('Launched', 'carl_ppo_return_merge'): 'last_strided rank',
                                       ('KeyError', "'mean'"): 'missing'},
                      'running.m2': {('ValueError', "ppo_return_merge running['m2']: needs a torch.float64 [1] tensor on cpu"): 'device dtype '
                                                                                                                                'last_dim',
                                     ('Launched', 'carl_ppo_return_merge'): 'last_strided rank',
                                     ('KeyError', "'m2'"): 'missing'},
                      'scale': {('ValueError', "ppo_return_merge 'scale': needs a float32 [1] tensor on cpu"): 'device dtype last_dim',
                                ('Launched', 'carl_ppo_return_merge'): 'last_strided rank'}},
 'ppo_adv_stats': {'advantage': {('ValueError', "ppo_adv_stats 'advantage': needs float32 [T, N] rows or a contiguous float32 [n] tensor on cpu"): 'device '
                                                                                                                                                   'dtype '
                                                                                                                                                   'rank',
                                 ('Launched', 'carl_ppo_adv_stats'): 'fewer_rows lanes last_dim more_rows pitch',
                                 ('ValueError', "ppo_adv_stats 'advantage': needs float32 [3, 24] rows of one pitch on cpu"): 'lane_strided '
                                                                                                                              'last_strided '
                                                                                                                              'pitch_zero'},
                   'idx': {('ValueError', "ppo_adv_stats 'idx': needs a contiguous int32 [n_total >= 1] tensor on cpu"): 'device dtype last_strided '
                                                                                                                         'rank',
                           ('Launched', 'carl_ppo_adv_stats'): 'fewer_rows last_dim'},
                   'out': {('ValueError', "ppo_adv_stats 'out': needs a contiguous float32 [3, 2] tensor on cpu"): 'device dtype fewer_rows '
                                                                                                                   'lane_strided lanes last_dim '
                                                                                                                   'last_strided more_rows pitch '
                                                                                                                   'pitch_zero rank'}},
 'ppo_adv_stats/flat': {'advantage': {('ValueError', "ppo_adv_stats 'advantage': needs float32 [T, N] rows or a contiguous float32 [n] tensor on cpu"): 'device '
                                                                                                                                                        'dtype '
                                                                                                                                                        'last_strided',
                                      ('Launched', 'carl_ppo_adv_stats'): 'fewer_rows last_dim rank'}},
 'ppo_adv_stats_sets': {'advantage': {('ValueError', "ppo_adv_stats_sets 'advantage': needs float32 [T, N] rows or a contiguous float32 [n] tensor on cpu"): 'device '
                                                                                                                                                             'dtype '
                                                                                                                                                             'rank',
                                      ('Launched', 'carl_ppo_adv_stats_sets'): 'fewer_rows lanes last_dim more_rows pitch',
                                      ('ValueError', "ppo_adv_stats_sets 'advantage': needs float32 [3, 24] rows of one pitch on cpu"): 'lane_strided '
                                                                                                                                        'last_strided '
                                                                                                                                        'pitch_zero'},
                        'idx': {('ValueError', "ppo_adv_stats_sets 'idx': needs int32 [P >= 1, n_total >= 1] rows of unit stride on cpu"): 'device '
                                                                                                                                           'dtype '
                                                                                                                                           'lane_strided '
                                                                                                                                           'last_strided '
                                                                                                                                           'pitch_zero '
                                                                                                                                           'rank',
                                ('Launched', 'carl_ppo_adv_stats_sets'): 'lanes last_dim pitch',
                                ('ValueError', "ppo_adv_stats_sets 'out': needs a contiguous float32 [1, 3, 2] tensor on cpu"): 'fewer_rows',
                                ('ValueError', "ppo_adv_stats_sets 'out': needs a contiguous float32 [3, 3, 2] tensor on cpu"): 'more_rows'},
                        'out': {('ValueError', "ppo_adv_stats_sets 'out': needs a contiguous float32 [2, 3, 2] tensor on cpu"): 'device dtype '
                                                                                                                                'fewer_rows '
                                                                                                                                'lane_strided lanes '
                                                                                                                                'last_dim '
                                                                                                                                'last_strided '
                                                                                                                                'more_rows pitch '
                                                                                                                                'pitch_zero rank'}},
 'ppo_adv_stats_sets/flat': {'advantage': {('ValueError', "ppo_adv_stats_sets 'advantage': needs float32 [T, N] rows or a contiguous float32 [n] tensor on cpu"): 'device '
                                                                                                                                                                  'dtype '
                                                                                                                                                                  'last_strided',
                                           ('Launched', 'carl_ppo_adv_stats_sets'): 'fewer_rows last_dim rank'}},
 'adam_step': {'params.0': {('ValueError', 'adam_step params[0]: needs a contiguous float32 tensor of 3 elements on cpu'): 'device dtype '
                                                                                                                           'last_strided',
                            ('Launched', 'carl_adam_step'): 'rank',
                            ('ValueError', 'adam_step grads[0]: needs a contiguous float32 tensor of 4 elements on cpu'): 'last_dim',
                            ('ValueError', 'adam_step grads[0]: needs a contiguous float32 tensor of 2 elements on cpu'): 'fewer_rows'},
               'params.1': {('ValueError', 'adam_step params[1]: needs a contiguous float32 tensor of 4 elements on cpu'): 'device dtype '
                                                                                                                           'lane_strided '
                                                                                                                           'last_strided pitch '
                                                                                                                           'pitch_zero',
                            ('Launched', 'carl_adam_step'): 'rank',
                            ('ValueError', 'adam_step grads[1]: needs a contiguous float32 tensor of 6 elements on cpu'): 'lanes last_dim more_rows',
                            ('ValueError', 'adam_step grads[1]: needs a contiguous float32 tensor of 2 elements on cpu'): 'fewer_rows'},
               'grads.1': {('ValueError', 'adam_step grads[1]: needs a contiguous float32 tensor of 4 elements on cpu'): 'device dtype fewer_rows '
                                                                                                                         'last_dim last_strided',
                           ('Launched', 'carl_adam_step'): 'rank'},
               'state.m.0': {('ValueError', "adam_step state['m'][0]: needs a contiguous float32 tensor of 3 elements on cpu"): 'device dtype '
                                                                                                                                'fewer_rows last_dim '
                                                                                                                                'last_strided',
                             ('Launched', 'carl_adam_step'): 'rank'},
               'state.v.1': {('ValueError', "adam_step state['v'][1]: needs a contiguous float32 tensor of 4 elements on cpu"): 'device dtype '
                                                                                                                                'fewer_rows '
                                                                                                                                'lane_strided lanes '
                                                                                                                                'last_dim '
                                                                                                                                'last_strided '
                                                                                                                                'more_rows pitch '
                                                                                                                                'pitch_zero',
                             ('Launched', 'carl_adam_step'): 'rank'},
               'state.step': {('ValueError', "adam_step state['step']: needs an int64 [1] tensor on cpu"): 'device dtype last_dim',
                              ('Launched', 'carl_adam_step'): 'last_strided rank',
                              ('KeyError', "'step'"): 'missing'},
               'state.beta_pow': {('ValueError', "adam_step state['beta_pow']: needs a contiguous float64 [2] tensor on cpu"): 'device dtype '
                                                                                                                               'fewer_rows last_dim '
                                                                                                                               'last_strided',
                                  ('Launched', 'carl_adam_step'): 'rank',
                                  ('KeyError', "'beta_pow'"): 'missing'},
               'norm_out': {('ValueError', "adam_step 'norm_out': needs a contiguous float64 [2] tensor on cpu"): 'device dtype fewer_rows last_dim '
                                                                                                                  'last_strided',
                            ('Launched', 'carl_adam_step'): 'rank'}},
 'adam_step_sets': {'params.0': {('ValueError', 'adam_step_sets params[0]: needs a contiguous float32 [2, 3] tensor on cpu'): 'device dtype '
                                                                                                                              'lane_strided '
                                                                                                                              'last_strided pitch '
                                                                                                                              'pitch_zero',
                                 ('ValueError', 'adam_step_sets grads[0]: needs a contiguous float32 [1, 6] tensor on cpu'): 'rank',
                                 ('ValueError', 'adam_step_sets grads[0]: needs a contiguous float32 [2, 4] tensor on cpu'): 'lanes last_dim',
                                 ('ValueError', 'adam_step_sets grads[0]: needs a contiguous float32 [1, 3] tensor on cpu'): 'fewer_rows',
                                 ('ValueError', 'adam_step_sets grads[0]: needs a contiguous float32 [3, 3] tensor on cpu'): 'more_rows'},
                    'params.1': {('ValueError', 'adam_step_sets params[1]: needs a contiguous float32 [2, 4] tensor on cpu'): 'device dtype '
                                                                                                                              'lane_strided '
                                                                                                                              'last_strided pitch '
                                                                                                                              'pitch_zero',
                                 ('ValueError', 'adam_step_sets params[1]: needs [2, n] rows, one per member'): 'fewer_rows more_rows rank',
                                 ('ValueError', 'adam_step_sets grads[1]: needs a contiguous float32 [2, 6] tensor on cpu'): 'lanes last_dim'},
                    'grads.1': {('ValueError', 'adam_step_sets grads[1]: needs a contiguous float32 [2, 4] tensor on cpu'): 'device dtype fewer_rows '
                                                                                                                            'lane_strided lanes '
                                                                                                                            'last_dim last_strided '
                                                                                                                            'more_rows pitch '
                                                                                                                            'pitch_zero rank'},
                    'state.m.0': {('ValueError', "adam_step_sets state['m'][0]: needs a contiguous float32 [2, 3] tensor on cpu"): 'device dtype '
                                                                                                                                   'fewer_rows '
                                                                                                                                   'lane_strided '
                                                                                                                                   'lanes last_dim '
                                                                                                                                   'last_strided '
                                                                                                                                   'more_rows pitch '
                                                                                                                                   'pitch_zero rank'},
                    'state.v.1': {('ValueError', "adam_step_sets state['v'][1]: needs a contiguous float32 [2, 4] tensor on cpu"): 'device dtype '
                                                                                                                                   'fewer_rows '
                                                                                                                                   'lane_strided '
                                                                                                                                   'lanes last_dim '
                                                                                                                                   'last_strided '
                                                                                                                                   'more_rows pitch '
                                                                                                                                   'pitch_zero rank'},
                    'state.step': {('ValueError', "adam_step_sets state['step']: needs a contiguous int64 [2] tensor on cpu"): 'device dtype '
                                                                                                                               'fewer_rows last_dim '
                                                                                                                               'last_strided rank',
                                   ('KeyError', "'step'"): 'missing'},
                    'state.beta_pow': {('ValueError', "adam_step_sets state['beta_pow']: needs a contiguous float64 [2, 2] tensor on cpu"): 'device '
                                                                                                                                            'dtype '
                                                                                                                                            'fewer_rows '
                                                                                                                                            'lane_strided '
                                                                                                                                            'lanes '
                                                                                                                                            'last_dim '
                                                                                                                                            'last_strided '
                                                                                                                                            'more_rows '
                                                                                                                                            'pitch '
                                                                                                                                            'pitch_zero '
                                                                                                                                            'rank',
                                       ('KeyError', "'beta_pow'"): 'missing'},
                    'norm_out': {('ValueError', "adam_step_sets 'norm_out': needs a contiguous float64 [2, 2] tensor on cpu"): 'device dtype '
                                                                                                                               'fewer_rows '
                                                                                                                               'lane_strided lanes '
                                                                                                                               'last_dim '
                                                                                                                               'last_strided '
                                                                                                                               'more_rows pitch '
                                                                                                                               'pitch_zero rank'},
                    'hyper': {('ValueError', "adam_step_sets 'hyper': needs a contiguous float64 [2, 5] tensor on cpu (columns lr, clip_range, vf_coef, ent_coef, max_grad_norm)"): 'device '
                                                                                                                                                                                    'dtype '
                                                                                                                                                                                    'fewer_rows '
                                                                                                                                                                                    'lane_strided '
                                                                                                                                                                                    'lanes '
                                                                                                                                                                                    'last_dim '
                                                                                                                                                                                    'last_strided '
                                                                                                                                                                                    'more_rows '
                                                                                                                                                                                    'pitch '
                                                                                                                                                                                    'pitch_zero '
                                                                                                                                                                                    'rank'}},
 'rollout_policy': {'out.obs': {('Launched', 'carl_rollout_policy_valued'): 'dtype more_rows',
                                ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'device',
                                ('ValueError', "rollout_policy output 'obs': shape (1, 3, 24, 4) / strides (384, 128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'rank',
                                ('ValueError', "rollout_policy output 'obs': shape (3, 24, 5) / strides (120, 5, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'last_dim',
                                ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (192, 8, 2) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'last_strided',
                                ('ValueError', "rollout_policy output 'obs': shape (2, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                ('ValueError', "rollout_policy output 'obs': shape (3, 25, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'lanes',
                                ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (256, 8, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'lane_strided',
                                ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (96, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'pitch',
                                ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (0, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'pitch_zero',
                                ('KeyError', "'obs'"): 'missing'},
                    'out.reward': {('Launched', 'carl_rollout_policy_valued'): 'dtype more_rows',
                                   ('ValueError', "rollout_policy output 'reward': shape (3, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'device',
                                   ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (24 lanes)"): 'pitch '
                                                                                                                                                                                        'pitch_zero '
                                                                                                                                                                                        'rank',
                                   ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (25 lanes)"): 'last_dim',
                                   ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (48 lanes)"): 'last_strided',
                                   ('ValueError', "rollout_policy output 'reward': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                   ('ValueError', "rollout_policy output 'reward': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                   ('ValueError', "rollout_policy output 'obs': shape (3, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (64 lanes)"): 'lane_strided',
                                   ('KeyError', "'reward'"): 'missing'},
                    'out.terminated': {('Launched', 'carl_rollout_policy_valued'): 'bool dtype more_rows',
                                       ('ValueError', "rollout_policy output 'terminated': shape (3, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'device',
                                       ('ValueError', "rollout_policy output 'terminated': shape (1, 3, 24) / strides (96, 32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'rank',
                                       ('ValueError', "rollout_policy output 'terminated': shape (3, 25) / strides (25, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_dim',
                                       ('ValueError', "rollout_policy output 'terminated': shape (3, 24) / strides (48, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_strided',
                                       ('ValueError', "rollout_policy output 'terminated': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                       ('ValueError', "rollout_policy output 'terminated': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                       ('ValueError', "rollout_policy output 'terminated': shape (3, 24) / strides (64, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lane_strided',
                                       ('ValueError', "rollout_policy output 'terminated': shape (3, 24) / strides (24, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch',
                                       ('ValueError', "rollout_policy output 'terminated': shape (3, 24) / strides (0, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch_zero',
                                       ('KeyError', "'terminated'"): 'missing'},
                    'out.truncated': {('Launched', 'carl_rollout_policy_valued'): 'bool dtype more_rows',
                                      ('ValueError', "rollout_policy output 'truncated': shape (3, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'device',
                                      ('ValueError', "rollout_policy output 'truncated': shape (1, 3, 24) / strides (96, 32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'rank',
                                      ('ValueError', "rollout_policy output 'truncated': shape (3, 25) / strides (25, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_dim',
                                      ('ValueError', "rollout_policy output 'truncated': shape (3, 24) / strides (48, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_strided',
                                      ('ValueError', "rollout_policy output 'truncated': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                      ('ValueError', "rollout_policy output 'truncated': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                      ('ValueError', "rollout_policy output 'truncated': shape (3, 24) / strides (64, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lane_strided',
                                      ('ValueError', "rollout_policy output 'truncated': shape (3, 24) / strides (24, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch',
                                      ('ValueError', "rollout_policy output 'truncated': shape (3, 24) / strides (0, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch_zero',
                                      ('KeyError', "'truncated'"): 'missing'},
                    'out.final_obs': {('Launched', 'carl_rollout_policy_valued'): 'dtype missing more_rows',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (3, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'device',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (1, 3, 24, 4) / strides (384, 128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'rank',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (3, 24, 5) / strides (120, 5, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'last_dim',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (3, 24, 4) / strides (192, 8, 2) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'last_strided',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (2, 24, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (3, 25, 4) / strides (128, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'lanes',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (3, 24, 4) / strides (256, 8, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'lane_strided',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (3, 24, 4) / strides (96, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'pitch',
                                      ('ValueError', "rollout_policy output 'final_obs': shape (3, 24, 4) / strides (0, 4, 1) do not form [>= 3, 24, 4] rows of one common pitch (32 lanes)"): 'pitch_zero'},
                    'out.action': {('ValueError', "rollout_policy 'action' buffer must be torch.int32 for this family"): 'dtype',
                                   ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'device',
                                   ('ValueError', "rollout_policy output 'action': shape (1, 3, 24) / strides (96, 32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'rank',
                                   ('ValueError', "rollout_policy output 'action': shape (3, 25) / strides (25, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_dim',
                                   ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (48, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_strided',
                                   ('ValueError', "rollout_policy output 'action': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                   ('Launched', 'carl_rollout_policy_valued'): 'more_rows',
                                   ('ValueError', "rollout_policy output 'action': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                   ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (64, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lane_strided',
                                   ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (24, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch',
                                   ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (0, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch_zero',
                                   ('ValueError', "rollout_policy output needs an 'action' [T, N] buffer"): 'missing'},
                    'out.log_prob': {('ValueError', "rollout_policy 'log_prob' buffer must be torch.float32"): 'dtype',
                                     ('ValueError', "rollout_policy 'log_prob' buffer must be on cpu"): 'device',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (1, 3, 24) / strides (96, 32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'rank',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (3, 25) / strides (25, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_dim',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (3, 24) / strides (48, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_strided',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                     ('Launched', 'carl_rollout_policy_valued'): 'missing more_rows',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (3, 24) / strides (64, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lane_strided',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (3, 24) / strides (24, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch',
                                     ('ValueError', "rollout_policy output 'log_prob': shape (3, 24) / strides (0, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch_zero'},
                    'out.value': {('ValueError', "rollout_policy 'value' buffer must be torch.float32"): 'dtype',
                                  ('ValueError', "rollout_policy 'value' buffer must be on cpu"): 'device',
                                  ('ValueError', "rollout_policy output 'value': shape (1, 3, 24) / strides (96, 32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'rank',
                                  ('ValueError', "rollout_policy output 'value': shape (3, 25) / strides (25, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_dim',
                                  ('ValueError', "rollout_policy output 'value': shape (3, 24) / strides (48, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_strided',
                                  ('ValueError', "rollout_policy output 'value': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                  ('Launched', 'carl_rollout_policy_valued'): 'missing more_rows',
                                  ('ValueError', "rollout_policy output 'value': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                  ('ValueError', "rollout_policy output 'value': shape (3, 24) / strides (64, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lane_strided',
                                  ('ValueError', "rollout_policy output 'value': shape (3, 24) / strides (24, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch',
                                  ('ValueError', "rollout_policy output 'value': shape (3, 24) / strides (0, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch_zero'},
                    'out.boot_value': {('ValueError', "rollout_policy 'boot_value' buffer must be torch.float32"): 'dtype',
                                       ('ValueError', "rollout_policy 'boot_value' buffer must be on cpu"): 'device',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (1, 3, 24) / strides (96, 32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'rank',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (3, 25) / strides (25, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_dim',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (3, 24) / strides (48, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_strided',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                       ('Launched', 'carl_rollout_policy_valued'): 'missing more_rows',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (3, 24) / strides (64, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lane_strided',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (3, 24) / strides (24, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch',
                                       ('ValueError', "rollout_policy output 'boot_value': shape (3, 24) / strides (0, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch_zero'},
                    'out.last_value': {('ValueError', "rollout_policy 'last_value' must be a contiguous float32 [24] tensor on cpu"): 'device dtype '
                                                                                                                                      'fewer_rows '
                                                                                                                                      'last_dim '
                                                                                                                                      'last_strided '
                                                                                                                                      'rank',
                                       ('Launched', 'carl_rollout_policy_valued'): 'missing'}},
 'rollout_policy/pendulum': {'out.action': {('ValueError', "rollout_policy 'action' buffer must be torch.float32 for this family"): 'dtype',
                                            ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'device',
                                            ('ValueError', "rollout_policy output 'action': shape (1, 3, 24) / strides (96, 32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'rank',
                                            ('ValueError', "rollout_policy output 'action': shape (3, 25) / strides (25, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_dim',
                                            ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (48, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'last_strided',
                                            ('ValueError', "rollout_policy output 'action': shape (2, 24) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'fewer_rows',
                                            ('Launched', 'carl_rollout_policy_valued'): 'more_rows',
                                            ('ValueError', "rollout_policy output 'action': shape (3, 25) / strides (32, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lanes',
                                            ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (64, 2) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'lane_strided',
                                            ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (24, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch',
                                            ('ValueError', "rollout_policy output 'action': shape (3, 24) / strides (0, 1) do not form [>= 3, 24] rows of one common pitch (32 lanes)"): 'pitch_zero',
                                            ('ValueError', "rollout_policy output needs an 'action' [T, N] buffer"): 'missing'}},
 'rollout_policy/brax': {'out.obs': {('Launched', 'carl_brax_rollout_policy_valued'): 'device dtype fewer_rows more_rows',
                                     ('ValueError', "rollout output 'obs': shape (1, 3, 8, 27) / strides (648, 216, 27, 1) do not form [T, 8, 27] rows of one common pitch (8 lanes)"): 'rank',
                                     ('ValueError', "rollout output 'obs': shape (3, 8, 28) / strides (224, 28, 1) do not form [T, 8, 27] rows of one common pitch (8 lanes)"): 'last_dim',
                                     ('ValueError', "rollout output 'obs': shape (3, 8, 27) / strides (432, 54, 2) do not form [T, 8, 27] rows of one common pitch (8 lanes)"): 'last_strided',
                                     ('ValueError', "rollout output 'obs': shape (3, 9, 27) / strides (243, 27, 1) do not form [T, 8, 27] rows of one common pitch (8 lanes)"): 'lanes',
                                     ('ValueError', "rollout output 'obs': shape (3, 8, 27) / strides (432, 54, 1) do not form [T, 8, 27] rows of one common pitch (8 lanes)"): 'lane_strided',
                                     ('ValueError', "rollout output 'obs': shape (3, 8, 27) / strides (648, 27, 1) do not form [T, 8, 27] rows of one common pitch (8 lanes)"): 'pitch',
                                     ('ValueError', "rollout output 'obs': shape (3, 8, 27) / strides (0, 27, 1) do not form [T, 8, 27] rows of one common pitch (8 lanes)"): 'pitch_zero',
                                     ('KeyError', "'obs'"): 'missing'},
                         'out.reward': {('Launched', 'carl_brax_rollout_policy_valued'): 'device dtype more_rows',
                                        ('ValueError', 'rollout output buffers are shorter than the action sequence'): 'fewer_rows rank',
                                        ('ValueError', 'BraxVecEngine: dense rows only (8 lanes per row); these output buffers have rows of 9 lanes'): 'lanes '
                                                                                                                                                       'last_dim',
                                        ('ValueError', 'BraxVecEngine: dense rows only (8 lanes per row); these output buffers have rows of 16 lanes'): 'lane_strided '
                                                                                                                                                        'last_strided',
                                        ('ValueError', 'BraxVecEngine: dense rows only (8 lanes per row); these output buffers have rows of 24 lanes'): 'pitch',
                                        ('ValueError', "rollout output 'reward': shape (3, 8) / strides (0, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'pitch_zero',
                                        ('KeyError', "'reward'"): 'missing'},
                         'out.terminated': {('Launched', 'carl_brax_rollout_policy_valued'): 'bool device dtype fewer_rows more_rows',
                                            ('ValueError', "rollout output 'terminated': shape (1, 3, 8) / strides (24, 8, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'rank',
                                            ('ValueError', "rollout output 'terminated': shape (3, 9) / strides (9, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'lanes '
                                                                                                                                                                                'last_dim',
                                            ('ValueError', "rollout output 'terminated': shape (3, 8) / strides (16, 2) do not form [T, 8] rows of one common pitch (8 lanes)"): 'lane_strided '
                                                                                                                                                                                 'last_strided',
                                            ('ValueError', "rollout output 'terminated': shape (3, 8) / strides (24, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'pitch',
                                            ('ValueError', "rollout output 'terminated': shape (3, 8) / strides (0, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'pitch_zero',
                                            ('KeyError', "'terminated'"): 'missing'},
                         'out.truncated': {('Launched', 'carl_brax_rollout_policy_valued'): 'bool device dtype fewer_rows more_rows',
                                           ('ValueError', "rollout output 'truncated': shape (1, 3, 8) / strides (24, 8, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'rank',
                                           ('ValueError', "rollout output 'truncated': shape (3, 9) / strides (9, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'lanes '
                                                                                                                                                                              'last_dim',
                                           ('ValueError', "rollout output 'truncated': shape (3, 8) / strides (16, 2) do not form [T, 8] rows of one common pitch (8 lanes)"): 'lane_strided '
                                                                                                                                                                               'last_strided',
                                           ('ValueError', "rollout output 'truncated': shape (3, 8) / strides (24, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'pitch',
                                           ('ValueError', "rollout output 'truncated': shape (3, 8) / strides (0, 1) do not form [T, 8] rows of one common pitch (8 lanes)"): 'pitch_zero',
                                           ('KeyError', "'truncated'"): 'missing'},
                         'out.action': {('ValueError', "rollout_policy output needs a contiguous float32 'action' [>= 3, 8, 8] buffer on cpu"): 'device '
                                                                                                                                                'dtype '
                                                                                                                                                'fewer_rows '
                                                                                                                                                'lane_strided '
                                                                                                                                                'lanes '
                                                                                                                                                'last_dim '
                                                                                                                                                'last_strided '
                                                                                                                                                'missing '
                                                                                                                                                'pitch '
                                                                                                                                                'pitch_zero '
                                                                                                                                                'rank',
                                        ('Launched', 'carl_brax_rollout_policy_valued'): 'more_rows'},
                         'out.log_prob': {('ValueError', "rollout_policy 'log_prob' buffer must be torch.float32"): 'dtype',
                                          ('ValueError', "rollout_policy 'log_prob' buffer must be on cpu"): 'device',
                                          ('ValueError', "rollout_policy output 'log_prob': shape (1, 3, 8) / strides (24, 8, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'rank',
                                          ('ValueError', "rollout_policy output 'log_prob': shape (3, 9) / strides (9, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'lanes '
                                                                                                                                                                                      'last_dim',
                                          ('ValueError', "rollout_policy output 'log_prob': shape (3, 8) / strides (16, 2) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'lane_strided '
                                                                                                                                                                                       'last_strided',
                                          ('ValueError', "rollout_policy output 'log_prob': shape (2, 8) / strides (8, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'fewer_rows',
                                          ('Launched', 'carl_brax_rollout_policy_valued'): 'missing more_rows',
                                          ('ValueError', "rollout_policy output 'log_prob': shape (3, 8) / strides (24, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'pitch',
                                          ('ValueError', "rollout_policy output 'log_prob': shape (3, 8) / strides (0, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'pitch_zero'},
                         'out.value': {('ValueError', "rollout_policy 'value' buffer must be torch.float32"): 'dtype',
                                       ('ValueError', "rollout_policy 'value' buffer must be on cpu"): 'device',
                                       ('ValueError', "rollout_policy output 'value': shape (1, 3, 8) / strides (24, 8, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'rank',
                                       ('ValueError', "rollout_policy output 'value': shape (3, 9) / strides (9, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'lanes '
                                                                                                                                                                                'last_dim',
                                       ('ValueError', "rollout_policy output 'value': shape (3, 8) / strides (16, 2) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'lane_strided '
                                                                                                                                                                                 'last_strided',
                                       ('ValueError', "rollout_policy output 'value': shape (2, 8) / strides (8, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'fewer_rows',
                                       ('Launched', 'carl_brax_rollout_policy_valued'): 'missing more_rows',
                                       ('ValueError', "rollout_policy output 'value': shape (3, 8) / strides (24, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'pitch',
                                       ('ValueError', "rollout_policy output 'value': shape (3, 8) / strides (0, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'pitch_zero'},
                         'out.boot_value': {('ValueError', "rollout_policy 'boot_value' buffer must be torch.float32"): 'dtype',
                                            ('ValueError', "rollout_policy 'boot_value' buffer must be on cpu"): 'device',
                                            ('ValueError', "rollout_policy output 'boot_value': shape (1, 3, 8) / strides (24, 8, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'rank',
                                            ('ValueError', "rollout_policy output 'boot_value': shape (3, 9) / strides (9, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'lanes '
                                                                                                                                                                                          'last_dim',
                                            ('ValueError', "rollout_policy output 'boot_value': shape (3, 8) / strides (16, 2) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'lane_strided '
                                                                                                                                                                                           'last_strided',
                                            ('ValueError', "rollout_policy output 'boot_value': shape (2, 8) / strides (8, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'fewer_rows',
                                            ('Launched', 'carl_brax_rollout_policy_valued'): 'missing more_rows',
                                            ('ValueError', "rollout_policy output 'boot_value': shape (3, 8) / strides (24, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'pitch',
                                            ('ValueError', "rollout_policy output 'boot_value': shape (3, 8) / strides (0, 1) do not form [>= 3, 8] rows of one common pitch (8 lanes)"): 'pitch_zero'},
                         'out.last_value': {('ValueError', "rollout_policy 'last_value' must be a contiguous float32 [8] tensor on cpu"): 'device '
                                                                                                                                          'dtype '
                                                                                                                                          'fewer_rows '
                                                                                                                                          'last_dim '
                                                                                                                                          'last_strided '
                                                                                                                                          'rank',
                                            ('Launched', 'carl_brax_rollout_policy_valued'): 'missing'}},
 'rollout_policy/summary': {'out.episodes': {('ValueError', "summary output 'episodes' must be a contiguous 4-byte [24] tensor on cpu"): 'device '
                                                                                                                                         'dtype '
                                                                                                                                         'fewer_rows '
                                                                                                                                         'last_dim '
                                                                                                                                         'last_strided',
                                             ('Launched', 'carl_rollout_policy'): 'rank',
                                             ('KeyError', "'episodes'"): 'missing'},
                            'out.return_sum': {('ValueError', "summary output 'return_sum' must be a contiguous 4-byte [24] tensor on cpu"): 'device '
                                                                                                                                             'dtype '
                                                                                                                                             'fewer_rows '
                                                                                                                                             'last_dim '
                                                                                                                                             'last_strided',
                                               ('Launched', 'carl_rollout_policy'): 'rank',
                                               ('KeyError', "'return_sum'"): 'missing'},
                            'out.length_sum': {('ValueError', "summary output 'length_sum' must be a contiguous 4-byte [24] tensor on cpu"): 'device '
                                                                                                                                             'dtype '
                                                                                                                                             'fewer_rows '
                                                                                                                                             'last_dim '
                                                                                                                                             'last_strided',
                                               ('Launched', 'carl_rollout_policy'): 'rank',
                                               ('KeyError', "'length_sum'"): 'missing'}},
 'rollout_policy/brax/summary': {'out.episodes': {('ValueError', "rollout_policy summary 'episodes' must be a contiguous torch.int32 [8] tensor on cpu"): 'device '
                                                                                                                                                          'dtype '
                                                                                                                                                          'fewer_rows '
                                                                                                                                                          'last_dim '
                                                                                                                                                          'last_strided '
                                                                                                                                                          'missing '
                                                                                                                                                          'rank'},
                                 'out.return_sum': {('ValueError', "rollout_policy summary 'return_sum' must be a contiguous torch.float32 [8] tensor on cpu"): 'device '
                                                                                                                                                                'dtype '
                                                                                                                                                                'fewer_rows '
                                                                                                                                                                'last_dim '
                                                                                                                                                                'last_strided '
                                                                                                                                                                'missing '
                                                                                                                                                                'rank'},
                                 'out.length_sum': {('ValueError', "rollout_policy summary 'length_sum' must be a contiguous torch.int32 [8] tensor on cpu"): 'device '
                                                                                                                                                              'dtype '
                                                                                                                                                              'fewer_rows '
                                                                                                                                                              'last_dim '
                                                                                                                                                              'last_strided '
                                                                                                                                                              'missing '
                                                                                                                                                              'rank'}},
 'evaluate_policy': {'out.episodes': {('ValueError', "evaluate_policy output 'episodes' must be a contiguous torch.int32 [24] tensor on cpu"): 'device '
                                                                                                                                               'dtype '
                                                                                                                                               'fewer_rows '
                                                                                                                                               'last_dim '
                                                                                                                                               'last_strided '
                                                                                                                                               'missing '
                                                                                                                                               'rank'},
                     'out.steps': {('ValueError', "evaluate_policy output 'steps' must be a contiguous torch.int32 [24] tensor on cpu"): 'device '
                                                                                                                                         'dtype '
                                                                                                                                         'fewer_rows '
                                                                                                                                         'last_dim '
                                                                                                                                         'last_strided '
                                                                                                                                         'missing '
                                                                                                                                         'rank'},
                     'out.return': {('ValueError', "evaluate_policy output 'return' must be a contiguous torch.float32 [2, 24] tensor on cpu"): 'device '
                                                                                                                                                'dtype '
                                                                                                                                                'fewer_rows '
                                                                                                                                                'lane_strided '
                                                                                                                                                'lanes '
                                                                                                                                                'last_dim '
                                                                                                                                                'last_strided '
                                                                                                                                                'missing '
                                                                                                                                                'more_rows '
                                                                                                                                                'pitch '
                                                                                                                                                'pitch_zero '
                                                                                                                                                'rank'},
                     'out.length': {('ValueError', "evaluate_policy output 'length' must be a contiguous torch.int32 [2, 24] tensor on cpu"): 'device '
                                                                                                                                              'dtype '
                                                                                                                                              'fewer_rows '
                                                                                                                                              'lane_strided '
                                                                                                                                              'lanes '
                                                                                                                                              'last_dim '
                                                                                                                                              'last_strided '
                                                                                                                                              'missing '
                                                                                                                                              'more_rows '
                                                                                                                                              'pitch '
                                                                                                                                              'pitch_zero '
                                                                                                                                              'rank'},
                     'out.context_id': {('ValueError', "evaluate_policy output 'context_id' must be a contiguous torch.int32 [2, 24] tensor on cpu"): 'device '
                                                                                                                                                      'dtype '
                                                                                                                                                      'fewer_rows '
                                                                                                                                                      'lane_strided '
                                                                                                                                                      'lanes '
                                                                                                                                                      'last_dim '
                                                                                                                                                      'last_strided '
                                                                                                                                                      'missing '
                                                                                                                                                      'more_rows '
                                                                                                                                                      'pitch '
                                                                                                                                                      'pitch_zero '
                                                                                                                                                      'rank'},
                     'out.terminated': {('ValueError', "evaluate_policy output 'terminated' must be a contiguous torch.uint8 [2, 24] tensor on cpu"): 'bool '
                                                                                                                                                      'device '
                                                                                                                                                      'dtype '
                                                                                                                                                      'fewer_rows '
                                                                                                                                                      'lane_strided '
                                                                                                                                                      'lanes '
                                                                                                                                                      'last_dim '
                                                                                                                                                      'last_strided '
                                                                                                                                                      'missing '
                                                                                                                                                      'more_rows '
                                                                                                                                                      'pitch '
                                                                                                                                                      'pitch_zero '
                                                                                                                                                      'rank'},
                     'out.input_partial': {('ValueError', "evaluate_policy output 'input_partial' must be a contiguous torch.float64 [1, 2, 32] tensor on cpu"): 'device '
                                                                                                                                                                 'dtype '
                                                                                                                                                                 'lane_strided '
                                                                                                                                                                 'lanes '
                                                                                                                                                                 'last_dim '
                                                                                                                                                                 'last_strided '
                                                                                                                                                                 'more_rows '
                                                                                                                                                                 'rank',
                                           ('Launched', 'carl_evaluate_policy_stats'): 'missing pitch pitch_zero'}},
 'evaluate_episodes': {'out.episodes': {('ValueError', "evaluate_episodes output 'episodes' must be a contiguous torch.int32 [8] tensor on cpu"): 'device '
                                                                                                                                                  'dtype '
                                                                                                                                                  'fewer_rows '
                                                                                                                                                  'last_dim '
                                                                                                                                                  'last_strided '
                                                                                                                                                  'missing '
                                                                                                                                                  'rank'},
                       'out.steps': {('ValueError', "evaluate_episodes output 'steps' must be a contiguous torch.int32 [8] tensor on cpu"): 'device '
                                                                                                                                            'dtype '
                                                                                                                                            'fewer_rows '
                                                                                                                                            'last_dim '
                                                                                                                                            'last_strided '
                                                                                                                                            'missing '
                                                                                                                                            'rank'},
                       'out.return': {('ValueError', "evaluate_episodes output 'return' must be a contiguous torch.float32 [2, 8] tensor on cpu"): 'device '
                                                                                                                                                   'dtype '
                                                                                                                                                   'fewer_rows '
                                                                                                                                                   'lane_strided '
                                                                                                                                                   'lanes '
                                                                                                                                                   'last_dim '
                                                                                                                                                   'last_strided '
                                                                                                                                                   'missing '
                                                                                                                                                   'more_rows '
                                                                                                                                                   'pitch '
                                                                                                                                                   'pitch_zero '
                                                                                                                                                   'rank'},
                       'out.length': {('ValueError', "evaluate_episodes output 'length' must be a contiguous torch.int32 [2, 8] tensor on cpu"): 'device '
                                                                                                                                                 'dtype '
                                                                                                                                                 'fewer_rows '
                                                                                                                                                 'lane_strided '
                                                                                                                                                 'lanes '
                                                                                                                                                 'last_dim '
                                                                                                                                                 'last_strided '
                                                                                                                                                 'missing '
                                                                                                                                                 'more_rows '
                                                                                                                                                 'pitch '
                                                                                                                                                 'pitch_zero '
                                                                                                                                                 'rank'},
                       'out.context_id': {('ValueError', "evaluate_episodes output 'context_id' must be a contiguous torch.int32 [2, 8] tensor on cpu"): 'device '
                                                                                                                                                         'dtype '
                                                                                                                                                         'fewer_rows '
                                                                                                                                                         'lane_strided '
                                                                                                                                                         'lanes '
                                                                                                                                                         'last_dim '
                                                                                                                                                         'last_strided '
                                                                                                                                                         'missing '
                                                                                                                                                         'more_rows '
                                                                                                                                                         'pitch '
                                                                                                                                                         'pitch_zero '
                                                                                                                                                         'rank'},
                       'out.terminated': {('ValueError', "evaluate_episodes output 'terminated' must be a contiguous torch.uint8 [2, 8] tensor on cpu"): 'bool '
                                                                                                                                                         'device '
                                                                                                                                                         'dtype '
                                                                                                                                                         'fewer_rows '
                                                                                                                                                         'lane_strided '
                                                                                                                                                         'lanes '
                                                                                                                                                         'last_dim '
                                                                                                                                                         'last_strided '
                                                                                                                                                         'missing '
                                                                                                                                                         'more_rows '
                                                                                                                                                         'pitch '
                                                                                                                                                         'pitch_zero '
                                                                                                                                                         'rank'},
                       'out.input_partial': {('ValueError', "evaluate_episodes output 'input_partial' must be a contiguous torch.float64 [0, 2, 32] tensor on cpu"): 'device '
                                                                                                                                                                     'dtype '
                                                                                                                                                                     'lanes '
                                                                                                                                                                     'last_dim '
                                                                                                                                                                     'more_rows '
                                                                                                                                                                     'rank',
                                             ('Launched', 'carl_brax_evaluate_policy_stats'): 'lane_strided last_strided missing pitch pitch_zero'}},
 'InputStats.update': {'policy_or_block': {('ValueError', 'InputStats.update: the block must be a contiguous float32 [148] or [n, 148] tensor on cpu'): 'device '
                                                                                                                                                        'dtype '
                                                                                                                                                        'lane_strided '
                                                                                                                                                        'lanes '
                                                                                                                                                        'last_dim '
                                                                                                                                                        'last_strided '
                                                                                                                                                        'pitch '
                                                                                                                                                        'pitch_zero '
                                                                                                                                                        'rank',
                                           ('Launched', 'carl_policy_stats_merge'): 'fewer_rows more_rows'}}}

RULES = {'rollout_policy/classic: gae without value_net': ('ValueError',
                                                   "gae=(gamma, lam) needs value_net: advantages are computed from the critic's values"),
 'rollout_policy/classic: value_net in summary mode': ('ValueError', "value_net: transitions mode only (mode='summary' stores nothing per step)"),
 'rollout_policy/classic: bootstrap_truncated without auto_reset': ('ValueError',
                                                                    'bootstrap_truncated=True needs auto_reset=True: without it no terminal '
                                                                    'observation is kept apart from the next one (pass bootstrap_truncated=False)'),
 'rollout_policy/classic: no bootstrap without auto_reset launches': ('Launched', 'carl_rollout_policy_valued'),
 'rollout_policy/classic: deterministic valued': ('Launched', 'carl_rollout_policy_valued'),
 'rollout_policy/classic: log_prob deterministic': ('ValueError', 'log_prob=True: sampled launches only (deterministic=False)'),
 'rollout_policy/classic: log_prob in summary mode': ('ValueError',
                                                      'log_prob=True: transitions mode only (a summary launch stores nothing per step)'),
 'rollout_policy/classic: summary without auto_reset': ('ValueError',
                                                        "mode='summary' needs auto_reset=True: without it a finished lane reports done on every "
                                                        'later step, and the totals would count its episode on each of them'),
 'rollout_policy/classic: unknown mode': ('ValueError', "mode 'episodes': 'transitions' or 'summary'"),
 'rollout_policy/classic: sampled with log_prob launches': ('Launched', 'carl_rollout_policy_sampled'),
 'rollout_policy/classic: summary launches': ('Launched', 'carl_rollout_policy'),
 'rollout_policy/classic: valued with gae launches': ('Launched', 'carl_rollout_policy_valued'),
 'rollout_policy/classic: gae of three values': ('ValueError', 'too many values to unpack (expected 2)'),
 'rollout_policy/classic: the actor as value_net': ('ValueError', "value_net must be an MLPPolicy built with head='value'"),
 'rollout_policy/classic: a critic as policy': ('ValueError', "the acting policy must have head='policy'"),
 'rollout_policy/classic: value_net of another transform': ('ValueError',
                                                            "value_net's input_shift / input_scale / input_clip must equal the policy's bit for bit: "
                                                            "the critic reads the actor's transformed inputs"),
 'rollout_policy/classic: out without action': ('ValueError', "rollout_policy output needs an 'action' [T, N] buffer"),
 'evaluate/classic: without auto_reset': ('ValueError',
                                          'evaluate_policy needs auto_reset=True: without it a finished lane reports done on every later step'),
 'evaluate/classic: no episodes': ('ValueError', 'n_episodes 0 < 1'),
 'evaluate/classic: negative steps': ('ValueError', 'max_steps -1 < 0'),
 'evaluate/classic: 2^31 records': ('ValueError', '2048 episodes x 1048576 lanes: more than 2^31 - 1 records'),
 'evaluate/classic: launches': ('Launched', 'carl_evaluate_policy'),
 'evaluate/classic: out without a key': ('ValueError', "evaluate_policy output 'episodes' must be a contiguous torch.int32 [24] tensor on cpu"),
 'alloc_policy_episodes/classic: no episodes': ('ValueError', 'n_episodes 0 < 1'),
 'rollout_policy/brax: gae without value_net': ('ValueError', "gae=(gamma, lam) needs value_net: advantages are computed from the critic's values"),
 'rollout_policy/brax: value_net in summary mode': ('ValueError', "value_net: transitions mode only (mode='summary' stores nothing per step)"),
 'rollout_policy/brax: bootstrap_truncated without auto_reset': ('ValueError',
                                                                 'bootstrap_truncated=True needs auto_reset=True: without it no terminal observation '
                                                                 'is kept apart from the next one (pass bootstrap_truncated=False)'),
 'rollout_policy/brax: no bootstrap without auto_reset launches': ('Launched', 'carl_brax_rollout_policy_valued'),
 'rollout_policy/brax: deterministic valued': ('ValueError',
                                               'value_net: sampled launches only (deterministic=False); a deterministic valued launch is not built '
                                               'for the Brax families'),
 'rollout_policy/brax: log_prob deterministic': ('ValueError', 'log_prob=True: sampled launches only (deterministic=False)'),
 'rollout_policy/brax: log_prob in summary mode': ('ValueError', 'log_prob=True: transitions mode only (a summary launch stores nothing per step)'),
 'rollout_policy/brax: summary without auto_reset': ('ValueError',
                                                     "mode='summary' needs auto_reset=True: without it a finished lane reports done on every later "
                                                     'step, and the totals would count its episode on each of them'),
 'rollout_policy/brax: unknown mode': ('ValueError', "mode 'episodes': 'transitions' or 'summary'"),
 'rollout_policy/brax: sampled with log_prob launches': ('Launched', 'carl_brax_rollout_policy_sampled'),
 'rollout_policy/brax: summary launches': ('Launched', 'carl_brax_rollout_policy'),
 'rollout_policy/brax: valued with gae launches': ('Launched', 'carl_brax_rollout_policy_valued'),
 'rollout_policy/brax: gae of three values': ('ValueError', 'too many values to unpack (expected 2)'),
 'rollout_policy/brax: the actor as value_net': ('ValueError',
                                                 "value_net must be a carl_amd.brax_policy.BraxMLPPolicy built with head='value' for this engine's "
                                                 'model (27 observations)'),
 'rollout_policy/brax: a critic as policy': ('ValueError',
                                             "the policy was built for 27 observations and 1 actuators, this engine's model has 27 and 8"),
 'rollout_policy/brax: value_net of another transform': ('ValueError',
                                                         "value_net's input_shift / input_scale / input_clip must equal the policy's bit for bit: "
                                                         "the critic reads the actor's transformed inputs"),
 'rollout_policy/brax: out without action': ('ValueError', "rollout_policy output needs a contiguous float32 'action' [>= 3, 8, 8] buffer on cpu"),
 'evaluate/brax: without auto_reset': ('ValueError',
                                       'evaluate_episodes needs auto_reset=True: without it a finished lane reports done on every later step'),
 'evaluate/brax: no episodes': ('ValueError', 'n_episodes 0 < 1'),
 'evaluate/brax: negative steps': ('ValueError', 'max_steps -1 < 0'),
 'evaluate/brax: 2^31 records': ('ValueError', '2048 episodes x 1048576 lanes: more than 2^31 - 1 records'),
 'evaluate/brax: launches': ('Launched', 'carl_brax_evaluate_policy'),
 'evaluate/brax: out without a key': ('ValueError', "evaluate_episodes output 'episodes' must be a contiguous torch.int32 [8] tensor on cpu"),
 'alloc_policy_episodes/brax: no episodes': ('ValueError', 'n_episodes 0 < 1'),
 'rollout_policy/classic: final_obs in summary mode': ('ValueError', 'final_obs: transitions mode only (a summary launch stores nothing per step)'),
 'rollout_policy/classic: summary out without a key': ('KeyError', "'episodes'"),
 'rollout_policy/brax: summary out without a key': ('ValueError',
                                                    "rollout_policy summary 'episodes' must be a contiguous torch.int32 [8] tensor on cpu"),
 'rollout_policy/classic: a Brax policy': ('ValueError', 'the policy was built for family -1, this engine runs family 0'),
 'rollout_policy/brax: a classic policy': ('TypeError', 'BraxVecEngine.rollout_policy takes a carl_amd.brax_policy.BraxMLPPolicy, not MLPPolicy'),
 'rollout_policy/brax: a classic critic': ('ValueError',
                                           "value_net must be a carl_amd.brax_policy.BraxMLPPolicy built with head='value' for this engine's model "
                                           '(27 observations)'),
 'rollout_policy/classic: value_net of another family': ('ValueError', 'value_net was built for family 2, the policy for family 0'),
 'rollout_policy/classic: value_net of other context rows': ('ValueError',
                                                             'value_net reads context rows [0], the policy [0, 1, 2, 3, 4, 5, 6, 7]: the critic sees '
                                                             "the actor's inputs"),
 'rollout_policy/classic: value_net of another set layout': ('ValueError',
                                                             'value_net has 1 weight sets of 256 lanes, the policy 1 of None: one set layout for '
                                                             'both'),
 'adam_state: no sets': ('ValueError', 'adam_state: n_sets 0 needs every parameter as [0, n] rows'),
 'adam_state: a parameter without the sets axis': ('ValueError', 'adam_state: n_sets 2 needs every parameter as [2, n] rows'),
 'adam_step: no tensors': ('ValueError', 'adam_step: 0 tensors, the launch takes 1 to 4'),
 'adam_step: five tensors': ('ValueError', 'adam_step: 5 tensors, the launch takes 1 to 4'),
 'adam_step: fewer gradients': ('ValueError', "adam_step: 2 parameters need 2 gradients and 2 entries of state['m'] / state['v']"),
 'adam_step_sets: no tensors': ('ValueError', 'adam_step_sets: 0 tensors, the launch takes 1 to 4'),
 'adam_step_sets: five tensors': ('ValueError', 'adam_step_sets: 5 tensors, the launch takes 1 to 4'),
 'adam_step_sets: fewer gradients': ('ValueError', "adam_step_sets: 2 parameters need 2 gradients and 2 entries of state['m'] / state['v']"),
 'adam_step_sets: params[0] a scalar': ('ValueError', 'adam_step_sets params[0]: needs [P, n] rows'),
 'adam_step_sets: params[1] of other sets': ('ValueError', 'adam_step_sets params[1]: needs [2, n] rows, one per member'),
 'adam_step_sets: hyper no tensor': ('ValueError',
                                     "adam_step_sets 'hyper': needs a contiguous float64 [2, 5] tensor on cpu (columns lr, clip_range, vf_coef, "
                                     'ent_coef, max_grad_norm)'),
 'ppo_adv_stats: batch_size 0': ('ValueError', 'ppo_adv_stats: batch_size 0 < 1'),
 'ppo_adv_stats_sets: batch_size 0': ('ValueError', 'ppo_adv_stats_sets: batch_size 0 < 1'),
 'ppo_adv_stats: a three-dimensional advantage': ('ValueError',
                                                  "ppo_adv_stats 'advantage': needs float32 [T, N] rows or a contiguous float32 [n] tensor on cpu"),
 'ppo_adv_stats_sets: an empty advantage': ('ValueError',
                                            "ppo_adv_stats_sets 'advantage': needs float32 [T, N] rows or a contiguous float32 [n] tensor on cpu"),
 'ppo_grad: idx None and no adv_norm launch': ('Launched', 'carl_ppo_grad'),
 'ppo_grad_sets: more samples than a member has': ('ValueError', "ppo_grad_sets 'idx': 769 samples per member, a member has 3 steps x 256 lanes"),
 'ppo_grad_sets: idx no tensor': ('ValueError', "ppo_grad_sets 'idx': needs int32 [2, M >= 1] rows of unit stride on cpu"),
 'ppo_grad_sets: no adv_norm launches': ('Launched', 'carl_ppo_grad_sets'),
 'ppo_grad_sets: actor and critic of other sets': ('ValueError',
                                                   'ppo_grad_sets: the actor and the critic need the same weight sets and lanes_per_set '
                                                   '(MLPPolicy.stack / on_device), got 2 x 256 and 1 x 512'),
 'ppo_grad_sets: sets that do not tile the lanes': ('ValueError',
                                                    "ppo_grad_sets: 2 sets x 256 lanes are not this engine's 768 lanes (member s owns lanes [s * "
                                                    'lanes_per_set, (s + 1) * lanes_per_set))'),
 'ppo_grad: a buffer of other lanes': ('ValueError', 'ppo_grad: a buffer of 24 lanes for an engine of 16'),
 'ppo_grad/brax: a classic policy': ('TypeError', 'BraxVecEngine.ppo_grad takes a carl_amd.brax_policy.BraxMLPPolicy, not MLPPolicy'),
 'ppo_input_stats: one step launches': ('Launched', 'carl_ppo_input_stats'),
 'ppo_input_stats: a one-dimensional context_id': ('ValueError', "ppo_input_stats 'context_id': needs int32 [T, 24] rows on cpu"),
 'ppo_input_stats: no steps': ('ValueError', 'ppo_input_stats: a buffer of 0 steps x 24 lanes for an engine of 24'),
 'ppo_input_stats: more slabs than needed launch': ('Launched', 'carl_ppo_input_stats'),
 'ppo_return_stats: without ret_rows launches': ('Launched', 'carl_ppo_return_stats'),
 'ppo_return_merge: scale allocated launches': ('Launched', 'carl_ppo_return_merge'),
 'ppo_workspace: no samples': ('ValueError', 'ppo_workspace: invalid shapes or n_samples 0'),
 'gae: buffers allocated launch': ('Launched', 'carl_gae'),
 'context_trace: out allocated launches': ('Launched', 'carl_policy_context_trace'),
 'context_trace/brax: padded rows': ('ValueError', 'BraxVecEngine.context_trace: dense rows only (8 lanes per row)'),
 'InputStats.update: block no tensor': ('ValueError', 'InputStats.update: the block must be a contiguous float32 [148] or [n, 148] tensor on cpu'),
 'InputStats.update: n_write beyond the block': ('ValueError', 'n_write 3 outside [0, 2]')}

